#!/usr/bin/env python3
"""Records tests/golden/early_formation.npz: per case of tests/test_gpu_early_formation.py the digest of one full sweep (mu, the
scalars, three rows and a checksum of Sigma and of Uv).  The fixture is the library's output BEFORE the masked groups were formed
one step early -- run this with that commit's csrc/libsgp_hip.so in place (same ABI), on the GPU:
    python tools/record_early_formation_golden.py [out.npz]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessnode_amd as G
from tests import test_gpu_early_formation as T

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
store = {}
for name in T.CASES:
    d, plans, first, second, full, resident, kinds = T.run_case(G, name)
    assert [g["form_step"] for g in plans[0]] == T.CASES[name]["form"], plans[0]
    T.assert_bitwise(second, first, name)
    T.assert_bitwise(full, first, name)
    T.assert_bitwise(resident, first, name)
    T.oracle_check(name, d, first)
    for k, v in T.digest(first, d).items():
        store[f"{name}/{k}"] = v
os.makedirs(os.path.dirname(out), exist_ok=True)
np.savez_compressed(out, **store)
print("wrote", out, os.path.getsize(out), "bytes")

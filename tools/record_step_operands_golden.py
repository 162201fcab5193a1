#!/usr/bin/env python3
"""Records tests/golden/step_operands_m{64,128,130,256}.npz: per case of tests/test_gpu_step_operands.py the digests (and, for
Q <= 128, the arrays) of one sweep, and the column a Lambda that is not positive definite reports.  The fixtures are the library's
output BEFORE the step kernel's MFMA runs read their operands a k-step ahead -- run this with that commit's csrc/libsgp_hip.so in
place (same ABI), on the GPU:
    python tools/record_step_operands_golden.py <commit the library was built from> [out dir]
The commit is written into every fixture (key `recorded_at`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessnode_amd as G
from tests import test_gpu_step_operands as T

commit = sys.argv[1]
out_dir = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN_DIR
os.makedirs(out_dir, exist_ok=True)


def setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = v


for M in T.SIZES:
    store = {"recorded_at": np.array(commit)}
    for mode in T.MODES:
        d, plan, snaps = T.run_case(G, M, mode, setenv)
        for s in snaps[1:]:
            for k in s:
                assert np.array_equal(s[k], snaps[0][k]), (M, mode, k)
        print(f"M={M} {mode}: form steps {[g['form_step'] for g in plan]} logdet_lambda {snaps[0]['logdet_lambda'][0]!r}")
        for k, v in T.record(d, plan, snaps[0]).items():
            store[f"{mode}/{k}"] = v
    for name, Mi, kind in T.INDEFINITE:
        if Mi == M:
            info = T.run_indefinite(G, M, kind, setenv)
            print(f"M={M} {name}: info {info}")
            assert info > 0, (name, info)
            store[f"indefinite/{name}"] = np.array([info], dtype=np.int64)
    path = os.path.join(out_dir, os.path.basename(T.golden_path(M)))
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")

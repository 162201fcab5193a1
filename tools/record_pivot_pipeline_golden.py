#!/usr/bin/env python3
"""Records tests/golden/pivot_pipeline_{m16,...,m200,indefinite,illcond}.npz: per case of tests/test_gpu_pivot_pipeline.py the
digests (and, for small M, the arrays) of one sweep and of one sgp_potrf factor, the column a non-positive pivot reports, and the
sweeps over an ill-conditioned K_uu.  The fixtures are the library's output BEFORE the pivot run of potf2_tile was software-
pipelined -- run this with that commit's csrc/libsgp_hip.so in place (same ABI), on the GPU:
    python tools/record_pivot_pipeline_golden.py <commit the library was built from> [out dir]
The commit is written into every fixture (key `recorded_at`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussianprocessnode_amd as G
from tests import test_gpu_pivot_pipeline as T

commit = sys.argv[1]
out_dir = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN_DIR
os.makedirs(out_dir, exist_ok=True)


def setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = v


def same_run_to_run(snaps, what):
    for s in snaps[1:]:
        for k in s:
            assert np.array_equal(s[k], snaps[0][k]), (what, k)


def write(name, store):
    path = os.path.join(out_dir, os.path.basename(T.golden_path(name)))
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


for M in T.SIZES:
    store = {"recorded_at": np.array(commit)}
    for mode in T.MODES:
        d, plan, snaps = T.run_case(G, M, mode, setenv)
        same_run_to_run(snaps, (M, mode))
        print(f"M={M} {mode}: form steps {[g['form_step'] for g in plan]} logdet_lambda {snaps[0]['logdet_lambda'][0]!r}")
        for k, v in T.record(d, plan, snaps[0]).items():
            store[f"{mode}/{k}"] = v
    A = T.spd_matrix(M, "potrf")
    L = G.potrf(A)
    assert np.array_equal(G.potrf(A), L), M
    print(f"M={M} potrf: |L L' - A| = {np.abs(L @ L.T - A).max():.3g}")
    for k, v in T.record_potrf(A, L).items():
        store[f"potrf/{k}"] = v
    write(f"m{M}", store)

store = {"recorded_at": np.array(commit)}
for c in T.BAD_COLUMNS:
    ip, isw = T.potrf_info(G, T.bad_matrix(c)), T.sweep_info(G, c, setenv)
    print(f"non-positive pivot at column {c}: sgp_potrf info {ip}, sweep info {isw}")
    assert ip == c + 1 and isw > 0, (c, ip, isw)
    store[f"potrf/col{c}"] = np.array([ip], dtype=np.int64)
    store[f"sweep/col{c}"] = np.array([isw], dtype=np.int64)
write("indefinite", store)

store = {"recorded_at": np.array(commit)}
for M, mode in T.ILL_CASES:
    d, plan, snaps = T.run_ill_case(G, M, mode, setenv)
    same_run_to_run(snaps, ("ill", M, mode))
    print(f"ill-conditioned M={M} {mode}: cond(K_uu) {T.cond_kuu(d['Xu'], T.ILL_ELL, T.ILL_JITTER):.3g} "
          f"logdet_kuu {snaps[0]['logdet_kuu'][0]!r}")
    for k, v in T.record(d, plan, snaps[0]).items():
        store[f"m{M}/{mode}/{k}"] = v
write("illcond", store)

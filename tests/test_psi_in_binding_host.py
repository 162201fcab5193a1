"""The exact-Psi input messages' boundary without a GPU: the entry point is declared in the header, exported, bound with its argument
types in _lib.py, and the new kernels are in the built library."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_point_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "sgp_hip.h")).read()
    from gaussianprocessnode_amd import _build, _lib
    blob = open(_build.build(), "rb").read()
    name = "sgp_psi_in_grad"
    assert re.search(r"int\s+%s\s*\(" % name, txt) and name in _lib.EXPORTS and name.encode() in blob
    fn = getattr(_lib.load(), name)
    dp = C.POINTER(C.c_double)
    assert list(fn.argtypes) == [C.c_void_p, dp, dp, dp, C.c_int64, dp, dp, dp, C.POINTER(C.c_int64)]
    for kernel in (b"k_psi_in_prep", b"k_psi_in_weights", b"k_psi2_in_accumulate", b"k_psi_in_finish"):
        assert kernel in blob, kernel
    from gaussianprocessnode_amd import SGPDevice, multisgp
    assert callable(SGPDevice.psi_in_grad) and callable(multisgp.marginal_in_exact_batch)

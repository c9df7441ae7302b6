"""Child process of tests/test_jln_tail_gpu.py::test_large_lds_orderings: the kernel cases named on the command line, in that
order, on the shipped library in a process that has launched nothing before - the large-LDS opt-in of
fvp_softargmax_weightnet is per-process state."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    import jln_tail_cases as T
    from faster_voxelpose_amd import _capi as capi
    lib = capi.load()
    for name in sys.argv[1:]:
        T.run_and_check_case(lib, "cuda:0", name, masks=False)
    print("ok: " + " ".join(sys.argv[1:]))

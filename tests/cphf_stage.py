"""mqc_hip_jk_multi_batch as a numpy-in / numpy-out function, the inputs of tests/test_gpu_jk_multi_stage.py, and its
child process: `python -m tests.cphf_stage N OUT.npz` runs the exact case of size N and writes J, K and the route (the
switch MQC_HIP_CPHF_MULTI is read once per process, so the other route needs a process of its own).  Test infrastructure."""
import ctypes as C
import sys

import numpy as np

from metalquicha_amd import capi
from tests import jk_stage_cases as jc

NFRAG, DONE = 3, 1          # fragments per call, and the one marked finished


def jk_multi_batch(tensor, D, done=None):
    """tensor (m, npair^2) square, D (m, nd, n, n) -> J, K (m, nd, n, n), NaN wherever the engine did not write, and
    the name of the instance chosen."""
    tensor = np.ascontiguousarray(tensor, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    m, nd, n = D.shape[0], D.shape[1], D.shape[-1]
    assert tensor.shape == (m, jc.npair(n) ** 2)
    J, K = np.full_like(D, np.nan), np.full_like(D, np.nan)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    route = C.create_string_buffer(64)
    capi.check(capi.load_library().mqc_hip_jk_multi_batch(
        capi.get_context(), m, n, nd, capi.dptr(tensor), capi.dptr(D), None if dn is None else dn.ctypes.data_as(capi.c_int32_p),
        capi.dptr(J), capi.dptr(K), route, len(route)))
    return J, K, route.value.decode()


def exact_inputs(n, nd=3):
    """NFRAG exact-integer fragments of size n with nd DIFFERENT densities each, one of them zero (nd >= 2): a kernel that
    mixes its accumulators cannot pass.  The finished fragment repeats the tensor of fragment 0."""
    Ms, Ds = [], []
    for f in range(NFRAG):
        M, Da = jc.exact_fragment(n, f) if f != DONE else (Ms[0], jc.exact_fragment(n, f, seed=31)[1])
        Dc = jc.exact_fragment(n, f, seed=99)[1] if n > 1 else Da + 1.0       # n = 1: one element, make it differ
        Ms.append(M)
        Ds.append(np.stack([Da, np.zeros_like(Da), Dc][:nd] if nd != 2 else [np.zeros_like(Da), Da]))
    return Ms, np.stack(Ds)


def run_exact(n, nd=3):
    Ms, D = exact_inputs(n, nd)
    done = np.zeros(NFRAG, dtype=np.int32)
    done[DONE] = 1
    T = np.stack([M.reshape(-1) for M in Ms])
    J, K, route = jk_multi_batch(T, D, done)
    return Ms, D, J, K, route


if __name__ == "__main__":
    _, _, J, K, route = run_exact(int(sys.argv[1]))
    np.savez(sys.argv[2], J=J, K=K, route=np.array(route))
    print(route)

"""mqc_hip_pcm_stage as a numpy-in / numpy-out function: the PCM stage of one fragment for a given density, with the
kernels of the SCF entry.  Test infrastructure (a ctypes helper for tests/), not part of the product package."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from metalquicha_amd import capi
from metalquicha_amd.methods import PcmSettings, PhysicalFragment, _Marshalled, _flat_basis


@dataclass
class PcmStage:
    tesserae: np.ndarray       # (T, 3) Bohr
    areas: np.ndarray          # (T,)
    A: np.ndarray              # (T, npair), pairs mu >= nu at mu (mu + 1) / 2 + nu
    v: np.ndarray              # (T,)
    q: np.ndarray              # (T,)
    e_pcm: float
    V: np.ndarray              # (n_ao, n_ao)


def pcm_stage_raw(basis_set: str, fragment: PhysicalFragment, pcm: PcmSettings, D: np.ndarray, tessera_capacity: int, a_capacity: int):
    """-> (status, T, PcmStage over arrays of the given capacities)"""
    m = _Marshalled(fragment, _flat_basis(basis_set, fragment))
    n = m.fb.nao
    npair = n * (n + 1) // 2
    keep: list = []
    popts = pcm.options(keep)
    D = np.ascontiguousarray(D, dtype=np.float64)
    T = C.c_int32(-1)
    e = C.c_double(0.0)
    tess, areas = np.full((max(tessera_capacity, 1), 3), np.nan), np.full(max(tessera_capacity, 1), np.nan)
    v, q = np.full(max(tessera_capacity, 1), np.nan), np.full(max(tessera_capacity, 1), np.nan)
    A = np.full(max(a_capacity, 1), np.nan)
    V = np.full((n, n), np.nan)
    rc = capi.load_library().mqc_hip_pcm_stage(capi.get_context(), C.byref(m.mol), C.byref(m.bas), C.byref(popts), capi.dptr(D),
                                               C.c_int32(tessera_capacity), C.c_int64(a_capacity), C.byref(T), capi.dptr(tess),
                                               capi.dptr(areas), capi.dptr(A), capi.dptr(v), capi.dptr(q), C.byref(e), capi.dptr(V))
    t = max(int(T.value), 0)
    out = None
    if rc == capi.MQC_HIP_OK:
        out = PcmStage(tess[:t].copy(), areas[:t].copy(), A[:t * npair].reshape(t, npair).copy(), v[:t].copy(), q[:t].copy(), float(e.value), V)
    return int(rc), int(T.value), out


def pcm_stage(basis_set: str, fragment: PhysicalFragment, pcm: PcmSettings, D: np.ndarray) -> PcmStage:
    """Two calls, as a caller that does not know T would make them: one for the count, one with the arrays."""
    n = _flat_basis(basis_set, fragment).nao
    lib = capi.load_library()
    m = _Marshalled(fragment, _flat_basis(basis_set, fragment))
    keep: list = []
    popts = pcm.options(keep)
    D = np.ascontiguousarray(D, dtype=np.float64)
    T = C.c_int32(0)
    capi.check(lib.mqc_hip_pcm_stage(capi.get_context(), C.byref(m.mol), C.byref(m.bas), C.byref(popts), capi.dptr(D), 0, 0,
                                     C.byref(T), None, None, None, None, None, None, None))
    rc, _, out = pcm_stage_raw(basis_set, fragment, pcm, D, int(T.value), int(T.value) * (n * (n + 1) // 2))
    capi.check(rc)
    return out

"""Stage-level entry points of the C ABI (mqc_hip_int1e, _eri_packed, _eri_packed_attenuated, _jk_incore, _jk_direct,
_coulomb_batch, _xc_batch, _df_jk_batch, _df_fit_batch, _jk_tensor_layout, _jk_incore_batch, _gradient_stage, _rimp2_stage, _syev,
_diis_coefficients) as numpy-in / numpy-out functions.  They run the same kernels the SCF
driver launches and exist so that each row of the hot-path table can be parity-tested alone.
Test infrastructure: a ctypes helper for tests/, not part of the product package."""
from __future__ import annotations

import ctypes as C

import numpy as np

from metalquicha_amd import capi
from metalquicha_amd.methods import PhysicalFragment, _Marshalled, _flat_basis


def _marshal(basis_set: str, fragment: PhysicalFragment):
    return _Marshalled(fragment, _flat_basis(basis_set, fragment))


def int1e(basis_set: str, fragment: PhysicalFragment):
    m = _marshal(basis_set, fragment)
    n = m.fb.nao
    S, T, V = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    capi.check(capi.load_library().mqc_hip_int1e(capi.get_context(), C.byref(m.mol), C.byref(m.bas),
                                                 capi.dptr(S), capi.dptr(T), capi.dptr(V)))
    return S, T, V


def eri_packed(basis_set: str, fragment: PhysicalFragment, schwarz_tol: float = 0.0) -> np.ndarray:
    m = _marshal(basis_set, fragment)
    n = m.fb.nao
    npair = n * (n + 1) // 2
    M = np.zeros((npair, npair))
    capi.check(capi.load_library().mqc_hip_eri_packed(capi.get_context(), C.byref(m.mol), C.byref(m.bas),
                                                      C.c_double(schwarz_tol), capi.dptr(M)))
    return M


def eri_packed_attenuated(basis_set: str, fragment: PhysicalFragment, omega: float, schwarz_tol: float = 0.0) -> np.ndarray:
    m = _marshal(basis_set, fragment)
    npair = m.fb.nao * (m.fb.nao + 1) // 2
    M = np.zeros((npair, npair))
    capi.check(capi.load_library().mqc_hip_eri_packed_attenuated(capi.get_context(), C.byref(m.mol), C.byref(m.bas),
                                                                 C.c_double(omega), C.c_double(schwarz_tol), capi.dptr(M)))
    return M


def jk_incore(basis_set: str, fragment: PhysicalFragment, D: np.ndarray):
    m = _marshal(basis_set, fragment)
    n = m.fb.nao
    D = np.ascontiguousarray(D, dtype=np.float64)
    J, K = np.zeros((n, n)), np.zeros((n, n))
    capi.check(capi.load_library().mqc_hip_jk_incore(capi.get_context(), C.byref(m.mol), C.byref(m.bas),
                                                     capi.dptr(D), capi.dptr(J), capi.dptr(K)))
    return J, K


def jk_direct(basis_set: str, fragment: PhysicalFragment, D: np.ndarray, schwarz_tol: float = 0.0, exx: float = 1.0):
    """mqc_hip_jk_direct: J and K by the direct digest kernels.  K comes back as all NaN where the engine did not write it."""
    m = _marshal(basis_set, fragment)
    n = m.fb.nao
    D = np.ascontiguousarray(D, dtype=np.float64)
    J, K = np.full((n, n), np.nan), np.full((n, n), np.nan)
    capi.check(capi.load_library().mqc_hip_jk_direct(capi.get_context(), C.byref(m.mol), C.byref(m.bas), C.c_double(schwarz_tol),
                                                     C.c_double(exx), capi.dptr(D), capi.dptr(J), capi.dptr(K)))
    return J, K


def syev(A: np.ndarray):
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    w, V = np.zeros(n), np.zeros((n, n))
    capi.check(capi.load_library().mqc_hip_syev(capi.get_context(), n, capi.dptr(A), capi.dptr(w), capi.dptr(V)))
    return w, V


def diis_coefficients(overlap: np.ndarray):
    B = np.ascontiguousarray(overlap, dtype=np.float64)
    n = B.shape[0]
    c = np.zeros(n)
    ok = C.c_int32(0)
    capi.check(capi.load_library().mqc_hip_diis_coefficients(capi.get_context(), n, capi.dptr(B), capi.dptr(c), C.byref(ok)))
    return c, bool(ok.value)


def pack_eri(eri4: np.ndarray) -> np.ndarray:
    """Full (n,n,n,n) tensor -> the engine's pair matrix layout, for comparisons."""
    n = eri4.shape[0]
    idx = [(i, j) for i in range(n) for j in range(i + 1)]
    ii = np.array([p[0] for p in idx]); jj = np.array([p[1] for p in idx])
    return eri4[ii[:, None], jj[:, None], ii[None, :], jj[None, :]]


def coulomb_batch(basis_set: str, fragments, D: np.ndarray, n_source_atoms: int = 0) -> np.ndarray:
    """mqc_hip_coulomb_batch for fragments of one element sequence: D (m, n, n) -> J (m, n, n)."""
    ms = [_marshal(basis_set, f) for f in fragments]
    mols = (capi.Molecule * len(ms))(*[m.mol for m in ms])
    D = np.ascontiguousarray(D, dtype=np.float64)
    J = np.zeros_like(D)
    capi.check(capi.load_library().mqc_hip_coulomb_batch(capi.get_context(), len(ms), mols, C.byref(ms[0].bas),
                                                         n_source_atoms, capi.dptr(D), capi.dptr(J)))
    return J


def xc_batch(basis_set: str, fragments, functional: str, D: np.ndarray, grid_level: int = 3, unrestricted: bool = False):
    """mqc_hip_xc_batch for fragments of one element sequence: D (m, n, n), or (m, 2, n, n) alpha then beta when
    unrestricted -> E_xc (m,), integrated electron number (m,), V_xc in the shape of D.  functional = None passes a
    null pointer (refusal tests)."""
    ms = [_marshal(basis_set, f) for f in fragments]
    mols = (capi.Molecule * max(1, len(ms)))(*[m.mol for m in ms])
    D = np.ascontiguousarray(D, dtype=np.float64)
    V = np.full_like(D, np.nan)
    e, nel = np.full(max(1, len(ms)), np.nan), np.full(max(1, len(ms)), np.nan)
    name = None if functional is None else functional.encode()
    capi.check(capi.load_library().mqc_hip_xc_batch(capi.get_context(), len(ms), mols, C.byref(ms[0].bas) if ms else None, name,
                                                    int(grid_level), 1 if unrestricted else 0, capi.dptr(D), capi.dptr(e), capi.dptr(nel),
                                                    capi.dptr(V)))
    return e, nel, V


def df_jk_batch(B: np.ndarray, D: np.ndarray, C_mo: np.ndarray, n_occ: int, exx: float = 1.0):
    """mqc_hip_df_jk_batch: B (m, n_aux, npair) packed pairs fastest, D and C (m, n, n) -> J, K (m, n, n) and the name
    of the kernel instance the dispatch chose.  J and K come back as NaN wherever the engine did not write."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    C_mo = np.ascontiguousarray(C_mo, dtype=np.float64)
    m, n = D.shape[0], D.shape[-1]
    assert B.shape[0] == m and B.shape[2] == n * (n + 1) // 2 and C_mo.shape == D.shape
    J, K = np.full_like(D, np.nan), np.full_like(D, np.nan)
    route = C.create_string_buffer(32)
    capi.check(capi.load_library().mqc_hip_df_jk_batch(capi.get_context(), m, n, int(n_occ), B.shape[1], C.c_double(exx), capi.dptr(B),
                                                       capi.dptr(D), capi.dptr(C_mo), capi.dptr(J), capi.dptr(K), route, len(route)))
    return J, K, route.value.decode()


def df_fit_batch(basis_set: str, aux_basis_set: str, fragments):
    """mqc_hip_df_fit_batch for fragments of one element sequence -> A3 (m, n_aux, npair), the metric (m, n_aux, n_aux),
    the fitted B (m, n_aux, npair), the fit flags (m,).  NaN wherever the engine did not write."""
    ms = [_marshal(basis_set, f) for f in fragments]
    xs = [_marshal(aux_basis_set, f) for f in fragments]
    mols = (capi.Molecule * len(ms))(*[m.mol for m in ms])
    m, n, na = len(ms), ms[0].fb.nao, xs[0].fb.nao
    npair = n * (n + 1) // 2
    A3, B = np.full((m, na, npair), np.nan), np.full((m, na, npair), np.nan)
    M, flag = np.full((m, na, na), np.nan), np.full(m, np.nan)
    capi.check(capi.load_library().mqc_hip_df_fit_batch(capi.get_context(), m, mols, C.byref(ms[0].bas), C.byref(xs[0].bas),
                                                        capi.dptr(A3), capi.dptr(M), capi.dptr(B), capi.dptr(flag)))
    return A3, M, B, flag


def jk_tensor_layout(n: int, nfrag: int, unrestricted: bool = False):
    """mqc_hip_jk_tensor_layout (host only, no context): (triangular, doubles per block, doubles per fragment) of the
    in-core tensor of an SCF batch of nfrag fragments of n functions."""
    tri, pb, stride = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
    capi.check(capi.load_library().mqc_hip_jk_tensor_layout(int(n), int(nfrag), 1 if unrestricted else 0, C.byref(tri), C.byref(pb),
                                                            C.byref(stride)))
    return bool(tri.value), pb.value, stride.value


def jk_incore_batch(tensor: np.ndarray, D: np.ndarray, unrestricted: bool = False, done=None, shell_l=None, Q=None, q_thresh: float = 0.0):
    """mqc_hip_jk_incore_batch: tensor (m, stride) as stored, D (m, n, n) -> J, K (m, n, n), loaded (m,), the name of the
    kernel instance the dispatch chose and the x extent of its grid.  J and K come back as NaN wherever the engine did
    not write.  done (m,): fragments marked finished (the launch then runs with only_active); shell_l, Q (m, ns, ns),
    q_thresh: the zero-row screening of the triangular kernel."""
    tensor = np.ascontiguousarray(tensor, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    m, n = D.shape[0], D.shape[-1]
    assert tensor.ndim == 2 and tensor.shape[0] == m
    J, K = np.full_like(D, np.nan), np.full_like(D, np.nan)
    loaded = np.full(m, -2, dtype=np.int32)
    route, gx = C.create_string_buffer(48), C.c_int32(0)
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    sl = None if shell_l is None else np.ascontiguousarray(shell_l, dtype=np.int32)
    q = None if Q is None else np.ascontiguousarray(Q, dtype=np.float64)
    capi.check(capi.load_library().mqc_hip_jk_incore_batch(
        capi.get_context(), m, n, 1 if unrestricted else 0, capi.dptr(tensor), tensor.shape[1], capi.dptr(D), None if dn is None else ip(dn),
        0 if sl is None else len(sl), None if sl is None else ip(sl), None if q is None else capi.dptr(q), C.c_double(q_thresh),
        capi.dptr(J), capi.dptr(K), ip(loaded), route, len(route), C.byref(gx)))
    return J, K, loaded, route.value.decode(), gx.value


RIMP2_ROUTE_FIELDS = ("clds", "npf", "waves", "oc", "gx", "lds", "napad", "nvpad", "npairs", "passes", "rows", "narrowed")


def rimp2_route(n: int, n_occ: int, n_aux: int, n_frozen: int = 0, m: int = 1, workgroups_per_fragment: int = 0) -> dict:
    """The host-only half of mqc_hip_rimp2_stage (no context, no device): the route the launcher of kern_mp2.hip takes for
    m fragments of this shape, as a dict over RIMP2_ROUTE_FIELDS."""
    route = np.full(16, -1, dtype=np.int32)
    capi.check(capi.load_library().mqc_hip_rimp2_stage(None, int(m), int(n), int(n_occ), int(n_aux), int(n_frozen),
                                                       int(workgroups_per_fragment), None, None, None, None, None, None, None, None,
                                                       route.ctypes.data_as(capi.c_int32_p)))
    return dict(zip(RIMP2_ROUTE_FIELDS, (int(v) for v in route)))


def rimp2_stage(B: np.ndarray, C_mo: np.ndarray, eps: np.ndarray, n_occ: int, n_frozen: int = 0, nmo=None, runs=None,
                workgroups_per_fragment: int = 0, want_bia: bool = True):
    """mqc_hip_rimp2_stage: B (m, n_aux, npair) packed pairs fastest, C (m, n, n), eps (m, n) -> e (m, 2), the pair
    partials (m, npairs, 2), Bia (m, no, napad, nvpad) with its padding (None unless want_bia) and the route as a dict.
    nmo, runs (m,): kept orbitals and the run flag of each fragment (default: n, 1).  Every output starts as NaN."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    C_mo = np.ascontiguousarray(C_mo, dtype=np.float64)
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    m, n = C_mo.shape[0], C_mo.shape[-1]
    assert B.shape[0] == m and B.shape[2] == n * (n + 1) // 2 and C_mo.shape == (m, n, n) and eps.shape == (m, n)
    nmo = np.full(m, n, dtype=np.int32) if nmo is None else np.ascontiguousarray(nmo, dtype=np.int32)
    runs = np.ones(m, dtype=np.int32) if runs is None else np.ascontiguousarray(runs, dtype=np.int32)
    no, napad, nvpad = n_occ - n_frozen, (B.shape[1] + 3) // 4 * 4, (n - n_occ + 15) // 16 * 16
    e, part = np.full((m, 2), np.nan), np.full((m, no * (no + 1) // 2, 2), np.nan)
    bia = np.full((m, no, napad, nvpad), np.nan) if want_bia else None
    route = np.full(16, -1, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    capi.check(capi.load_library().mqc_hip_rimp2_stage(capi.get_context(), m, n, int(n_occ), B.shape[1], int(n_frozen),
                                                       int(workgroups_per_fragment), capi.dptr(B), capi.dptr(C_mo), capi.dptr(eps), ip(nmo),
                                                       ip(runs), capi.dptr(e), capi.dptr(part), None if bia is None else capi.dptr(bia),
                                                       ip(route)))
    rt = dict(zip(RIMP2_ROUTE_FIELDS, (int(v) for v in route)))
    assert (rt["napad"], rt["nvpad"], rt["npairs"]) == (napad, nvpad, part.shape[1])
    return e, part, bia, rt


def unpack_pairs(P: np.ndarray) -> np.ndarray:
    """(..., npair) packed pairs (mu >= nu, index mu (mu + 1) / 2 + nu) -> the symmetric (..., n, n)."""
    npair = P.shape[-1]
    n = int((np.sqrt(8 * npair + 1) - 1) / 2)
    ii, jj = np.tril_indices(n)
    out = np.zeros(P.shape[:-1] + (n, n), dtype=P.dtype)
    out[..., ii, jj] = P
    out[..., jj, ii] = P
    return out


GRAD_EXACT, GRAD_DF3C, GRAD_DF2C = 0, 1, 2


def gradient_rows(basis_set: str, fragment: PhysicalFragment, cls, start: int = 0, count: int = 1, mode: int = GRAD_EXACT,
                  aux_basis_set: str | None = None):
    """The host-only half of mqc_hip_gradient_stage (no context, no device): rows [start, start + count) of the list of
    class cls = (la, lb, lc, ld) as the engine holds it, and the length of that list.  count = None: the whole list."""
    m = _marshal(basis_set, fragment)
    x = _marshal(aux_basis_set, fragment) if aux_basis_set else None
    lib = capi.load_library()

    def call(first, cnt):
        a = capi.GradientStage()
        a.mode = mode
        a.row_class[:] = [int(v) for v in cls]
        a.row_start, a.row_count = first, cnt
        rows = np.full((cnt, 4), -1, dtype=np.int32)
        length = C.c_int64(-1)
        a.rows = rows.ctypes.data_as(capi.c_int32_p)
        a.class_length = C.pointer(length)
        capi.check(lib.mqc_hip_gradient_stage(None, C.byref(m.mol), C.byref(m.bas), C.byref(x.bas) if x else None, C.byref(a)))
        return rows, length.value
    if count is not None:
        return call(start, count)
    out, length = call(0, 1)
    parts = [call(k, min(4096, length - k))[0] for k in range(0, length, 4096)]
    return np.concatenate(parts), length


def gradient_stage(basis_set: str, fragment: PhysicalFragment, D=None, D_beta=None, C_mo=None, eps=None, C_beta=None, eps_beta=None,
                   n_occ: int = 0, n_beta: int = 0, exx: float = 1.0, want=(), pair=None, Q=None, q_thresh: float = 0.0,
                   cls=None, start: int = 0, count: int = 0, mode: int = GRAD_EXACT, aux_basis_set: str | None = None, gam=None,
                   context=True, out=None):
    """mqc_hip_gradient_stage for one fragment.  want: any of "w", "g1e", "g2e"; pair = (A, B) adds "g1e_pair"; cls with
    count > 0 adds "rows" (count, 4), "class_length" and "g_rows" (count, natoms, 3).  Every output starts as NaN (rows as
    -1) and comes back so wherever the engine did not write; a caller's `out` dict receives them even when the call raises."""
    m = _marshal(basis_set, fragment)
    x = _marshal(aux_basis_set, fragment) if aux_basis_set else None
    n, nat = m.fb.nao, len(fragment.element_numbers)
    keep = []

    def dbl(v):
        if v is None:
            return None
        v = np.ascontiguousarray(v, dtype=np.float64)
        keep.append(v)
        return capi.dptr(v)
    a = capi.GradientStage()
    a.D, a.D_beta, a.C, a.eps, a.C_beta, a.eps_beta = dbl(D), dbl(D_beta), dbl(C_mo), dbl(eps), dbl(C_beta), dbl(eps_beta)
    a.n_occ, a.n_beta, a.exx = int(n_occ), int(n_beta), float(exx)
    a.Q, a.q_thresh, a.gam, a.mode = dbl(Q), float(q_thresh), dbl(gam), int(mode)
    out = {} if out is None else out
    for name, shape in (("w", (n, n)), ("g1e", (nat, 3)), ("g2e", (nat, 3))):
        if name in want:
            out[name] = np.full(shape, np.nan)
            setattr(a, name, capi.dptr(out[name]))
    a.pair_a = a.pair_b = -1
    if pair is not None:
        a.pair_a, a.pair_b = int(pair[0]), int(pair[1])
        out["g1e_pair"] = np.full((nat, 3), np.nan)
        a.g1e_pair = capi.dptr(out["g1e_pair"])
    length = C.c_int64(-1)
    if cls is not None:
        a.row_class[:] = [int(v) for v in cls]
        a.row_start, a.row_count = int(start), int(count)
        out["rows"] = np.full((max(count, 0), 4), -1, dtype=np.int32)
        out["g_rows"] = np.full((max(count, 0), nat, 3), np.nan)
        a.rows = out["rows"].ctypes.data_as(capi.c_int32_p)
        a.g_rows = capi.dptr(out["g_rows"])
        a.class_length = C.pointer(length)
    capi.check(capi.load_library().mqc_hip_gradient_stage(capi.get_context() if context else None, C.byref(m.mol), C.byref(m.bas),
                                                          C.byref(x.bas) if x else None, C.byref(a)))
    out["class_length"] = length.value
    return out

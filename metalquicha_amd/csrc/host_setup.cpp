// host_setup.cpp -- host-side preparation below the C ABI: contraction normalisation,
// topology (shell, pair and quartet-class lists), the Boys table and cart->sph tables, and the
// device layout of a batch chunk (carve_chunk: the one place every per-fragment array is sized).
// Nothing here computes integrals or any part of an SCF; that is all on the device.
#include "driver.hpp"
#include "md_integrals.hpp"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <sstream>

namespace mqc {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) { g_last_error = msg; return code; }
const std::string& last_error_string() { return g_last_error; }

// ---- device pool ---------------------------------------------------------------------
namespace {
struct PoolRegistry {
    std::mutex m;
    std::vector<DevicePool*> pools;
};
PoolRegistry& pool_registry() { static PoolRegistry* r = new PoolRegistry(); return *r; }   // never destroyed: pools may outlive statics
}  // namespace

DevicePool::DevicePool()
{
    auto& r = pool_registry();
    std::lock_guard<std::mutex> lock(r.m);
    r.pools.push_back(this);
}

DevicePool::~DevicePool()
{
    auto& r = pool_registry();
    std::lock_guard<std::mutex> lock(r.m);
    r.pools.erase(std::remove(r.pools.begin(), r.pools.end(), this), r.pools.end());
    // device memory is released by mqc_hip_finalize (release_all_pools); at process exit the runtime reclaims it
}

void release_all_pools()
{
    auto& r = pool_registry();
    std::lock_guard<std::mutex> lock(r.m);
    for (DevicePool* p : r.pools) p->release();
}

void* DevicePool::ensure(size_t bytes)
{
    if (bytes <= cap_ && ptr_) return ptr_;
    if (ptr_) { (void)hipFree(ptr_); ptr_ = nullptr; cap_ = 0; }
    size_t want = bytes + bytes / 8 + 256;     // a little headroom so near-equal batches do not realloc
    if (hipMalloc(&ptr_, want) != hipSuccess) {
        ptr_ = nullptr; cap_ = 0;
        if (hipMalloc(&ptr_, bytes) != hipSuccess) { ptr_ = nullptr; return nullptr; }
        want = bytes;
    }
    cap_ = want;
    return ptr_;
}

void DevicePool::release()
{
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr; cap_ = 0;
}

// ---- Boys table: F_0..F_{BOYS_COLS-1} on the grid T0 = r * BOYS_STEP --------------------
static void boys_series(int nmax, double T, double* F)
{
    if (T < 1e-13) { for (int n = 0; n <= nmax; ++n) F[n] = 1.0 / (2 * n + 1) - T / (2 * n + 3); return; }
    const double et = std::exp(-T);
    long double term = 1.0L / (2 * nmax + 1), sum = term;
    for (int k = 1; k < 600; ++k) {
        term *= 2.0L * T / (2 * nmax + 2 * k + 1);
        sum += term;
        if (term < 1e-20L * sum) break;
    }
    F[nmax] = (double)(et * sum);
    for (int n = nmax; n > 0; --n) F[n - 1] = (2.0 * T * F[n] + et) / (2 * n - 1);
}

void build_boys_table(std::vector<double>& table)
{
    table.assign((size_t)BOYS_ROWS * BOYS_COLS, 0.0);
    std::vector<double> F(BOYS_COLS + 1);
    for (int r = 0; r < BOYS_ROWS; ++r) {
        boys_series(BOYS_COLS - 1, r * BOYS_STEP, F.data());
        for (int c = 0; c < BOYS_COLS; ++c) table[(size_t)r * BOYS_COLS + c] = F[c];
    }
}

// ---- real solid harmonics r^l Y_lm in libcint's order (m = -l..l; p = x,y,z) ------------
static double binom(int n, int k)
{
    if (k < 0 || k > n) return 0.0;
    double r = 1.0;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return r;
}
static double fact(int n) { double r = 1.0; for (int i = 2; i <= n; ++i) r *= i; return r; }

void build_c2s_tables(std::vector<double>& packed, int* offsets)
{
    packed.clear();
    for (int l = 0; l <= LMAX_AO; ++l) {
        offsets[l] = (int)packed.size();
        const int nc = ncart(l), ns = nsph(l);
        std::vector<double> tab((size_t)ns * nc, 0.0);
        std::vector<int> cx, cy, cz;
        for (int lx = l; lx >= 0; --lx)
            for (int ly = l - lx; ly >= 0; --ly) { cx.push_back(lx); cy.push_back(ly); cz.push_back(l - lx - ly); }
        const double to_y = std::sqrt((2.0 * l + 1.0) / (4.0 * M_PI));
        for (int m = -l; m <= l; ++m) {
            const int am = std::abs(m);
            const double nlm = 1.0 / (std::pow(2.0, am) * fact(l)) *
                               std::sqrt(2.0 * fact(l + am) * fact(l - am) / (m == 0 ? 2.0 : 1.0));
            const int twov0 = (m >= 0) ? 0 : 1;
            for (int t = 0; t <= (l - am) / 2; ++t)
                for (int u = 0; u <= t; ++u)
                    for (int twov = twov0; twov <= am; twov += 2) {
                        const int sp = t + (twov - twov0) / 2;
                        const double c = ((sp & 1) ? -1.0 : 1.0) * std::pow(0.25, t) * binom(l, t) *
                                         binom(l - t, am + t) * binom(t, u) * binom(am, twov);
                        const int ex = 2 * t + am - 2 * u - twov, ey = 2 * u + twov, ez = l - 2 * t - am;
                        if (ex < 0 || ey < 0 || ez < 0) continue;
                        for (int k = 0; k < nc; ++k)
                            if (cx[k] == ex && cy[k] == ey && cz[k] == ez) tab[(size_t)(m + l) * nc + k] += nlm * c * to_y;
                    }
        }
        if (l <= 1) {
            // s and p: the constant is folded into the contraction coefficients, identity here
            std::fill(tab.begin(), tab.end(), 0.0);
            for (int k = 0; k < nc; ++k) tab[(size_t)k * nc + k] = 1.0;
        }
        packed.insert(packed.end(), tab.begin(), tab.end());
    }
}

// ---- contraction normalisation (mqc_libcint_integrals.F90:519-555) ----------------------
static double gto_norm(int l, double a)
{
    const int n = 2 * l + 2;
    const double gint = std::tgamma((n + 1) / 2.0) / (2.0 * std::pow(2.0 * a, (n + 1) / 2.0));
    return 1.0 / std::sqrt(gint);
}

std::string topology_key(const mqc_hip_molecule_t& mol, const mqc_hip_basis_t& bas)
{
    std::ostringstream os;
    os << mol.n_atoms << ':' << mol.nelec << ':' << mol.charge << ':' << mol.multiplicity << ':';
    for (int i = 0; i < mol.n_atoms; ++i)
        os << mol.atomic_numbers[i] << (mol.ghost && mol.ghost[i] ? 'g' : 'r') << bas.nshell_per_atom[i] << ',';
    os << '|' << bas.n_shells << '|';
    size_t off = 0;
    // the basis content: hash of the raw bytes so that two different sets with equal shapes differ
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void* p, size_t nbytes) {
        const unsigned char* b = (const unsigned char*)p;
        for (size_t i = 0; i < nbytes; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    };
    for (int s = 0; s < bas.n_shells; ++s) {
        os << bas.shell_l[s] << '.' << bas.shell_nprim[s] << ',';
        mix(bas.exponents + off, sizeof(double) * bas.shell_nprim[s]);
        mix(bas.coefficients + off, sizeof(double) * bas.shell_nprim[s]);
        off += bas.shell_nprim[s];
    }
    os << '#' << h;
    return os.str();
}

int build_topology(const mqc_hip_molecule_t& mol, const mqc_hip_basis_t& bas, Topology& topo, std::string& err, int max_l,
                   bool with_quartets)
{
    if (mol.n_atoms <= 0) { err = "fragment has no atoms"; return MQC_HIP_ERR_VALIDATION; }
    if (bas.n_atoms != mol.n_atoms) { err = "the basis covers a different number of atoms than the geometry has"; return MQC_HIP_ERR_VALIDATION; }
    if (!bas.spherical) {
        err = "Cartesian basis sets are not supported by the HIP backend (spherical only)";
        return MQC_HIP_ERR_UNSUPPORTED;
    }
    topo = Topology();
    topo.key = topology_key(mol, bas);
    topo.natoms = mol.n_atoms;
    topo.nelec = mol.nelec; topo.charge = mol.charge; topo.multiplicity = mol.multiplicity;
    topo.Z.assign(mol.atomic_numbers, mol.atomic_numbers + mol.n_atoms);
    topo.zeff.resize(mol.n_atoms);
    for (int i = 0; i < mol.n_atoms; ++i) topo.zeff[i] = (mol.ghost && mol.ghost[i]) ? 0.0 : (double)mol.atomic_numbers[i];

    constexpr double S_FACTOR = 0.282094791773878143, P_FACTOR = 0.488602511902919921;
    size_t poff_in = 0;
    int sh = 0, aoff = 0;
    for (int at = 0; at < mol.n_atoms; ++at) {
        for (int64_t k = 0; k < bas.nshell_per_atom[at]; ++k, ++sh) {
            if (sh >= bas.n_shells) { err = "nshell_per_atom does not sum to n_shells"; return MQC_HIP_ERR_VALIDATION; }
            const int l = bas.shell_l[sh], np = bas.shell_nprim[sh];
            if (l < 0 || l > LMAX_AO) { err = "angular momentum above g is not supported"; return MQC_HIP_ERR_UNSUPPORTED; }
            if (l > max_l) {
                err = "this build of the HIP backend covers angular momentum up to l = " + std::to_string(max_l) +
                      (max_l == KERNEL_LMAX ? " for orbital shells" : " for auxiliary shells");
                return MQC_HIP_ERR_UNSUPPORTED;
            }
            if (np <= 0) { err = "shell without primitives"; return MQC_HIP_ERR_VALIDATION; }
            const double* a = bas.exponents + poff_in;
            const double* c = bas.coefficients + poff_in;
            std::vector<double> cn(np);
            for (int i = 0; i < np; ++i) {
                if (!(a[i] > 0.0)) { err = "non-positive exponent"; return MQC_HIP_ERR_VALIDATION; }
                cn[i] = c[i] * gto_norm(l, a[i]);
            }
            double norm2 = 0.0;
            for (int i = 0; i < np; ++i)
                for (int j = 0; j < np; ++j)
                    norm2 += cn[i] * cn[j] / (gto_norm(l, a[i]) * gto_norm(l, a[j])) *
                             std::pow(2.0 * std::sqrt(a[i] * a[j]) / (a[i] + a[j]), l + 1.5);
            const double scale = norm2 > 0.0 ? 1.0 / std::sqrt(norm2) : 1.0;
            const double ang = (l == 0) ? S_FACTOR : (l == 1 ? P_FACTOR : 1.0);
            HostShell hs;
            hs.l = l; hs.atom = at; hs.aoff = aoff; hs.poff = (int)topo.exps.size(); hs.nprim = 0;
            for (int i = 0; i < np; ++i) {
                if (c[i] == 0.0) continue;     // a zero row entry of a general contraction contributes nothing
                topo.exps.push_back(a[i]);
                topo.coefs.push_back(cn[i] * scale * ang);
                hs.nprim++;
            }
            if (hs.nprim == 0) { err = "shell with all-zero coefficients"; return MQC_HIP_ERR_VALIDATION; }
            topo.shells.push_back(hs);
            topo.lmax = std::max(topo.lmax, l);
            aoff += 2 * l + 1;
            poff_in += np;
        }
    }
    if (sh != bas.n_shells) { err = "nshell_per_atom does not sum to n_shells"; return MQC_HIP_ERR_VALIDATION; }
    topo.nao = aoff;
    topo.npair = aoff * (aoff + 1) / 2;

    // shell pairs A >= B
    const int ns = (int)topo.shells.size();
    for (int A = 0; A < ns; ++A)
        for (int B = 0; B <= A; ++B) { topo.pairs.push_back(A); topo.pairs.push_back(B); }

    if (!with_quartets) return MQC_HIP_OK;     // auxiliary bases and density-fitted runs need no quartet lists
    // canonical quartets: pair index ab >= cd; inside a pair the higher l first; bra class >= ket class
    struct P { int a, b, la, lb, pc, np; };
    std::vector<P> pl;
    for (int A = 0; A < ns; ++A)
        for (int B = 0; B <= A; ++B) {
            int a = A, b = B;
            if (topo.shells[a].l < topo.shells[b].l) std::swap(a, b);
            const int la = topo.shells[a].l, lb = topo.shells[b].l;
            pl.push_back({a, b, la, lb, la * (la + 1) / 2 + lb, topo.shells[a].nprim * topo.shells[b].nprim});
        }
    std::map<int, Topology::ClassList> cls;
    std::map<int, std::vector<std::pair<int, std::array<int, 4>>>> tmp;   // class -> (cost, quartet)
    for (size_t ij = 0; ij < pl.size(); ++ij)
        for (size_t kl = 0; kl <= ij; ++kl) {
            P bra = pl[ij], ket = pl[kl];
            if (bra.pc < ket.pc) std::swap(bra, ket);
            const int id = ((bra.la * 8 + bra.lb) * 8 + ket.la) * 8 + ket.lb;
            tmp[id].push_back({bra.np * ket.np, {bra.a, bra.b, ket.a, ket.b}});
            topo.n_quartets++;
        }
    // ---- twin s shells: consecutive s shells of one atom contracted over identical primitives
    topo.twin_first.assign(ns, 0);
    std::vector<int> member_of_twin(ns, 0);
    for (int A = 0; A + 1 < ns; ++A) {
        const HostShell &x = topo.shells[A], &y = topo.shells[A + 1];
        if (member_of_twin[A] || x.l != 0 || y.l != 0 || x.atom != y.atom || x.nprim != y.nprim || x.nprim < 2) continue;
        bool same = true;
        for (int k = 0; k < x.nprim; ++k) same = same && (topo.exps[x.poff + k] == topo.exps[y.poff + k]);
        if (!same) continue;
        topo.twin_first[A] = 1;
        member_of_twin[A] = member_of_twin[A + 1] = 1;
    }
    // super-shells (a twin pair counts once), their canonical pairs and quartets -> twin entries per class
    std::map<int, std::vector<std::pair<int, std::array<int, 4>>>> ttmp;
    {
        std::vector<int> sup;     // first member of every super-shell
        for (int A = 0; A < ns; ++A) if (!(member_of_twin[A] && !topo.twin_first[A])) sup.push_back(A);
        struct SP { int a, b, la, lb, pc, np; };
        std::vector<SP> spl;
        for (size_t X = 0; X < sup.size(); ++X)
            for (size_t Y = 0; Y <= X; ++Y) {
                int a = sup[X], b = sup[Y];
                if (topo.shells[a].l < topo.shells[b].l) std::swap(a, b);
                const int la = topo.shells[a].l, lb = topo.shells[b].l;
                spl.push_back({a, b, la, lb, la * (la + 1) / 2 + lb, topo.shells[a].nprim * topo.shells[b].nprim});
            }
        for (size_t ij = 0; ij < spl.size(); ++ij)
            for (size_t kl = 0; kl <= ij; ++kl) {
                SP bra = spl[ij], ket = spl[kl];
                if (bra.pc < ket.pc) std::swap(bra, ket);
                if (!eri_has_twin_block(bra.la, bra.lb, ket.la, ket.lb)) continue;
                const int sh4[4] = {bra.a, bra.b, ket.a, ket.b};
                if (!(topo.twin_first[sh4[0]] || topo.twin_first[sh4[1]] || topo.twin_first[sh4[2]] || topo.twin_first[sh4[3]])) continue;
                std::array<int, 4> e;
                for (int k = 0; k < 4; ++k) e[k] = sh4[k] | (topo.twin_first[sh4[k]] ? (1 << 16) : 0);
                const int id = ((bra.la * 8 + bra.lb) * 8 + ket.la) * 8 + ket.lb;
                ttmp[id].push_back({bra.np * ket.np, e});
            }
    }
    for (auto& kv : tmp) {
        auto& v = kv.second;
        // deepest contractions first: lanes of a wave then share a trip count even in a batch of one
        std::stable_sort(v.begin(), v.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
        Topology::ClassList cl;
        const int id = kv.first;
        cl.ld = id % 8; cl.lc = (id / 8) % 8; cl.lb = (id / 64) % 8; cl.la = id / 512;
        for (auto& q : v) for (int k = 0; k < 4; ++k) cl.quartets.push_back(q.second[k]);
        if (eri_has_twin_block(cl.la, cl.lb, cl.lc, cl.ld) && ttmp.count(id)) {
            auto& tv = ttmp[id];
            std::stable_sort(tv.begin(), tv.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
            for (auto& q : tv) for (int k = 0; k < 4; ++k) cl.twin_entries.push_back(q.second[k]);
            for (auto& q : v) {
                const auto& e = q.second;
                if (member_of_twin[e[0]] || member_of_twin[e[1]] || member_of_twin[e[2]] || member_of_twin[e[3]]) continue;
                for (int k = 0; k < 4; ++k) cl.rest.push_back(e[k]);
            }
        }
        topo.classes.push_back(std::move(cl));
    }
    // atom set of every list entry (block sharing between fragments of a batch, kern_eri.hip)
    {
        std::map<std::vector<int>, int> ids;
        auto set_of = [&](const int* e) {
            std::vector<int> a(4);
            for (int k = 0; k < 4; ++k) a[k] = topo.shells[e[k] & 0xffff].atom;
            std::sort(a.begin(), a.end());
            a.erase(std::unique(a.begin(), a.end()), a.end());
            auto it = ids.find(a);
            if (it != ids.end()) return it->second;
            const int id = (int)topo.atom_sets.size();
            ids.emplace(a, id);
            topo.atom_sets.push_back(a);
            return id;
        };
        for (auto& cl : topo.classes) {
            for (size_t q = 0; q + 3 < cl.quartets.size(); q += 4) cl.set_quartets.push_back(set_of(&cl.quartets[q]));
            for (size_t q = 0; q + 3 < cl.twin_entries.size(); q += 4) cl.set_twin.push_back(set_of(&cl.twin_entries[q]));
            for (size_t q = 0; q + 3 < cl.rest.size(); q += 4) cl.set_rest.push_back(set_of(&cl.rest[q]));
        }
    }
    return MQC_HIP_OK;
}

// ---- device layout of a batch ------------------------------------------------------------
// doubles per block: the padded long triangle plus the padded short one, worst row pair (even, so that blocks stay
// 16-byte aligned); optionally where the short row starts in every block
int jk_tri_block(int np, std::vector<int>* short_row_start)
{
    auto shell_row = [](int idx) { int k = (int)((std::sqrt(8.0 * idx + 1.0) - 1.0) * 0.5); while ((k + 1) * (k + 2) / 2 <= idx) ++k; while (k * (k + 1) / 2 > idx) --k; return k; };
    const int npairs = (np + 1) / 2;
    // table: [npairs] start of the short row in every block, then [np] the shell row i of every pair row (ij)
    if (short_row_start) {
        short_row_start->assign((size_t)npairs + np, 0);
        for (int r = 0; r < np; ++r) (*short_row_start)[(size_t)npairs + r] = shell_row(r);
    }
    int worst = 0;
    for (int t = 0; t < npairs; ++t) {
        const int rl = np - 1 - t, il = shell_row(rl), is = shell_row(t);
        const int sb = (il + 1) * (il + 2) / 2;
        const int need = sb + (t < rl ? (is + 1) * (is + 2) / 2 : 0);
        if (short_row_start) (*short_row_start)[t] = sb;
        if (need > worst) worst = need;
    }
    return (worst + 1) & ~1;
}

size_t jk_tri_lds_bytes(int n, int np)
{
    // row buffers, packed D' and J (+ 2), Kh; zero-row flags, function -> shell map, per-wave maxima
    return sizeof(double) * ((size_t)JK_TRI_NW * jk_tri_block(np) + 2 * ((size_t)np + 2) + (size_t)n * n) + (((size_t)np + 15) & ~(size_t)15) + 64 * sizeof(int) + JK_TRI_NW * sizeof(double);
}

// The triangular layout is taken for the batches the tuned square kernel served: restricted, dimer-sized fragments
// (n <= 64, a multiple of 8; 640 < npair; a block within ten chunks of 128) in batches of at least 64.
// MQC_HIP_ERI_TRI=0: the square.
bool jk_tri_layout(int n, int np, int nfrag, bool uhf)
{
    static const bool on = env_on("MQC_HIP_ERI_TRI");
    if (!on || uhf || nfrag < 64 || n > 64 || n % 8 != 0 || np <= 10 * 64) return false;
    if (jk_tri_block(np) > JK_TRI_MAXU2 * 128) return false;
    return jk_tri_lds_bytes(n, np) <= (size_t)160 * 1024 - 1024;
}

void plan_layout(BatchPlan& p, int ntot, int nshell, int lmax, bool rad_cache)
{
    p.eri_tri = p.two_e == TWO_E_INCORE && !p.square_only && jk_tri_layout(p.n, p.npair, ntot, p.uhf);
    // radial cache of the quadrature: 2 doubles per shell and (padded) grid point; point buffer of the split quadrature
    // (n <= 96, s-f shells, 32-point tiles): 4 doubles per padded grid point
    p.rad_pt = xc_tile_points(p.n);
    const size_t tiles = p.xc.ncomp > 0 ? ((size_t)p.npts + p.rad_pt - 1) / p.rad_pt : 0;
    p.rad_doubles = (p.xc.ncomp > 0 && rad_cache && !p.uhf) ? tiles * (size_t)nshell * 2 * p.rad_pt : 0;
    p.pt4_doubles = (p.rad_doubles && p.n <= 96 && lmax <= 3 && p.rad_pt == 32) ? tiles * p.rad_pt * 4 : 0;
}

ChunkBytes carve_chunk(const BatchPlan& p, int nfrag, char* const* bases, BatchView& bv, std::vector<CarvedArray>* record, PcmView* pcm)
{
    const size_t nf = (size_t)nfrag, n = (size_t)p.n, nn = n * n, np = (size_t)p.npair;
    ChunkBytes used;
    auto take = [&](int pool, size_t bytes) -> void* {
        const uintptr_t at = (uintptr_t)(bases ? bases[pool] : nullptr) + used.pool[pool];
        used.pool[pool] += (bytes + 255) & ~size_t(255);
        if (record) record->push_back({pool, (const void*)at, bytes});
        return (void*)at;
    };
    auto doubles = [&](int pool, size_t count) { return (double*)take(pool, sizeof(double) * count); };
    bv.nfrag = nfrag; bv.n = p.n; bv.npair = p.npair; bv.uhf = p.uhf ? 1 : 0; bv.npc = p.npc; bv.naux = p.naux;

    // the SCF matrices: S H X F D C J K, W = 6 work matrices, the DIIS histories; beta spin: D C F J K Vprev, histories
    bv.xyz = doubles(POOL_MAIN, nf * p.natoms * 3);
    for (double** m : {&bv.S, &bv.H, &bv.X, &bv.F, &bv.D, &bv.C, &bv.J, &bv.K}) *m = doubles(POOL_MAIN, nf * nn);
    bv.W = doubles(POOL_MAIN, nf * 6 * nn);
    bv.Vprev = doubles(POOL_MAIN, nf * nn);
    bv.diis_f = doubles(POOL_MAIN, nf * DIIS_MAX * nn);
    bv.diis_e = doubles(POOL_MAIN, nf * DIIS_MAX * nn);
    bv.diis_b = doubles(POOL_MAIN, nf * DIIS_MAX * DIIS_MAX);
    bv.eps = doubles(POOL_MAIN, nf * n);
    bv.scal = doubles(POOL_MAIN, nf * 8);
    bv.dip = doubles(POOL_MAIN, nf * 4);
    bv.Db = bv.Cb = bv.Fb = bv.Jb = bv.Kb = bv.Vprevb = bv.epsb = bv.diis_fb = bv.diis_eb = nullptr;
    if (p.uhf) {
        for (double** m : {&bv.Db, &bv.Cb, &bv.Fb, &bv.Jb, &bv.Kb, &bv.Vprevb}) *m = doubles(POOL_MAIN, nf * nn);
        bv.diis_fb = doubles(POOL_MAIN, nf * DIIS_MAX * nn);
        bv.diis_eb = doubles(POOL_MAIN, nf * DIIS_MAX * nn);
        bv.epsb = doubles(POOL_MAIN, nf * n);
    }
    bv.diis_state = (int*)take(POOL_MAIN, sizeof(int) * nf * 2);
    bv.istate = (int*)take(POOL_MAIN, sizeof(int) * nf * 4);
    // embedding: the point charges (x, y, z, q), the operator U, the caller's h_extra
    bv.pc = p.npc > 0 ? doubles(POOL_MAIN, nf * p.npc * 4) : nullptr;
    bv.U = (p.npc > 0 || p.hx) ? doubles(POOL_MAIN, nf * nn) : nullptr;
    bv.Hx = p.hx ? doubles(POOL_MAIN, nf * nn) : nullptr;

    // counters (the quartet count of the integral stage at int 16); a triangular tensor's block table and read counters
    bv.counters = (int*)take(POOL_MISC, 256);
    bv.eri_count = (unsigned long long*)(bv.counters + 16);
    bv.eri_tri = p.eri_tri ? 1 : 0;
    bv.eri_tri_pb = p.eri_tri ? jk_tri_block(p.npair) : 0;
    bv.eri_tri_sb = p.eri_tri ? (const int*)take(POOL_MISC, sizeof(int) * ((np + 1) / 2 + np)) : nullptr;
    bv.jk_loaded = p.eri_tri ? (int*)take(POOL_MISC, sizeof(int) * nf) : nullptr;

    // the in-core tensor, square or in triangular blocks; a range-separated hybrid's tensor of erf(omega r12)/r12 in
    // the same layout, the J scratch of its J/K stream and K_lr of each spin
    const bool incore = p.two_e == TWO_E_INCORE;
    bv.eri_stride = !incore ? 0 : p.eri_tri ? (np + 1) / 2 * (size_t)bv.eri_tri_pb : np * np;
    bv.eri = incore ? doubles(POOL_ERI, nf * bv.eri_stride) : nullptr;
    const bool lr = incore && p.rsh;
    bv.eri_lr = lr ? doubles(POOL_ERI, nf * bv.eri_stride) : nullptr;
    bv.Jlr = lr ? doubles(POOL_ERI, nf * nn) : nullptr;
    bv.Klr = lr ? doubles(POOL_ERI, nf * nn) : nullptr;
    bv.Klrb = lr && p.uhf ? doubles(POOL_ERI, nf * nn) : nullptr;

    // Kohn-Sham: grid weights, the V_xc accumulator of each spin, radial cache, point buffer
    const bool ks = p.xc.ncomp > 0;
    bv.grid.weights = ks ? doubles(POOL_GRIDW, nf * p.npts) : nullptr;
    bv.Vxc = (ks || p.pcm_stride > 0) ? doubles(POOL_GRIDW, nf * nn * (p.uhf ? 2 : 1)) : nullptr;
    bv.grid.rad = ks && p.rad_doubles ? doubles(POOL_GRIDW, nf * p.rad_doubles) : nullptr;
    bv.grid.pt4 = ks && p.pt4_doubles ? doubles(POOL_GRIDW, nf * p.pt4_doubles) : nullptr;
    if (ks) bv.grid.rad_pt = p.rad_pt;

    // density fitting: (P|mu nu), the fitted tensor, the metric, its inverse root and the fit's scratch
    const bool df = p.two_e == TWO_E_DF;
    const size_t a3 = nf * p.naux * np, mm = nf * p.naux * p.naux;
    bv.df_a3 = df ? doubles(POOL_DF, a3) : nullptr;
    bv.df_b = df ? doubles(POOL_DF, a3) : nullptr;
    bv.df_metric = df ? doubles(POOL_DF, mm) : nullptr;
    bv.df_linv = df ? doubles(POOL_DF, mm) : nullptr;
    bv.df_work = df ? doubles(POOL_DF, mm) : nullptr;

    // C-PCM: tesserae, cavity matrix with its inverse factor and scratch, A and B = L^-1 A, the vectors, the packed density
    if (p.pcm_stride > 0) {
        PcmView pv;
        const size_t ts = (size_t)p.pcm_stride;
        pv.stride = p.pcm_stride; pv.f = p.pcm_f;
        pv.nt = (int*)take(POOL_PCM, sizeof(int) * nf);
        pv.pts = doubles(POOL_PCM, nf * ts * 4);
        for (double** m : {&pv.S, &pv.Linv, &pv.work}) *m = doubles(POOL_PCM, nf * ts * ts);
        pv.A = doubles(POOL_PCM, nf * ts * np);
        pv.B = doubles(POOL_PCM, nf * ts * np);
        for (double** m : {&pv.vnuc, &pv.b, &pv.c, &pv.v}) *m = doubles(POOL_PCM, nf * ts);
        pv.dp = doubles(POOL_PCM, nf * np);
        pv.scal = doubles(POOL_PCM, nf * 8);
        if (pcm) *pcm = pv;
    }
    return used;
}

// ---- C-PCM: the settings' and a molecule's refusals, then the cavity (pcm_cavity.hpp)
int pcm_check_options(const mqc_hip_pcm_options_t* o, std::string& msg)
{
    if (!o) { msg = "PCM: null options"; return MQC_HIP_ERR_VALIDATION; }
    if (!std::isfinite(o->epsilon) || o->epsilon < 1.0) { msg = "PCM: the dielectric constant epsilon must be finite and at least 1 (1 is the vacuum)"; return MQC_HIP_ERR_VALIDATION; }
    if (pcm::rule_index(o->angular_points) < 0) {
        msg = "PCM: angular_points = " + std::to_string(o->angular_points) + " is not a Lebedev rule of the engine up to 590 points "
              "(38, 50, 74, 86, 110, 146, 170, 194, 230, 266, 302, 350, 434, 590)";
        return MQC_HIP_ERR_VALIDATION;
    }
    if (!std::isfinite(o->radius_scale) || !(o->radius_scale > 0.0)) { msg = "PCM: radius_scale must be positive and finite"; return MQC_HIP_ERR_VALIDATION; }
    return MQC_HIP_OK;
}

int pcm_build_cavity(const mqc_hip_molecule_t& mol, const mqc_hip_pcm_options_t& o, pcm::Cavity& cav, std::string& msg)
{
    if (mol.n_point_charges > 0) { msg = "PCM: a fragment that carries external point charges is not supported (the charges would have to polarise the continuum too)"; return MQC_HIP_ERR_UNSUPPORTED; }
    if (mol.h_extra) { msg = "PCM: a fragment that carries an extra one-electron operator (h_extra) is not supported"; return MQC_HIP_ERR_UNSUPPORTED; }
    std::vector<double> rho;
    if (!pcm::sphere_radii(mol.n_atoms, mol.atomic_numbers, mol.ghost, o.radius_scale, o.radii_by_z, rho, msg)) return MQC_HIP_ERR_VALIDATION;
    for (int k = 0; k < 3 * mol.n_atoms; ++k)
        if (!std::isfinite(mol.xyz[k])) { msg = "PCM: a non-finite coordinate"; return MQC_HIP_ERR_VALIDATION; }
    if (!pcm::build_cavity(mol.n_atoms, mol.xyz, rho.data(), o.angular_points, cav, msg)) return MQC_HIP_ERR_VALIDATION;
    if (cav.count < 1) { msg = "PCM: the fragment has no real atom, so no cavity"; return MQC_HIP_ERR_VALIDATION; }
    return MQC_HIP_OK;
}

size_t fragment_bytes(const BatchPlan& p)
{
    BatchView probe{};
    // each array of nf fragments is rounded up to 256 bytes once, so a chunk never needs more than nf single fragments;
    // the direct path's launcher keeps its J and K accumulators in pools of its own
    return carve_chunk(p, 1, nullptr, probe).total() + (p.two_e == TWO_E_DIRECT ? sizeof(double) * 2 * (size_t)p.n * p.n : 0);
}

int64_t stage_chunk_fragments(size_t free_bytes, size_t per_fragment_bytes, int64_t nfrag, int64_t cap)
{
    return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nfrag, cap), (int64_t)((double)free_bytes * 0.7 / (double)per_fragment_bytes)));
}

size_t batch_budget_bytes(size_t free_b, size_t reservation, int lane, size_t hbm_budget)
{
    // a lane shares the card with the other lane's batch: 40 % each instead of 80 %
    size_t budget = (size_t)((lane < 0 ? 0.80 : 0.40) * (double)free_b);
    // ... and the pools never take what the runtime's scratch reservation may need (engine.cpp, scratch_reservation_bytes)
    const size_t room = free_b > reservation ? free_b - reservation : free_b / 8;
    const size_t cap = lane < 0 ? room : room / 2;
    if (cap < budget) budget = cap;
    if (hbm_budget && hbm_budget < budget) budget = hbm_budget;
    return budget;
}

// Small batches run as one chunk on lane 0.  Large ones are cut into >= pipeline_chunks chunks that alternate between
// the two lanes (each lane may hold half of the budget).
long batch_chunk_fragments(size_t budget, size_t per_frag, int ntot, int lane, int pipeline_chunks, int pipeline_min_fragments)
{
    const bool pipelined = lane < 0 && pipeline_chunks > 1 && ntot >= pipeline_min_fragments;
    long chunk = (long)(budget / per_frag);
    if (lane < 0 && (pipelined || chunk < ntot)) {
        // more than one chunk: two are resident at a time
        chunk = (long)(budget / 2 / per_frag);
        const long want = pipelined ? (ntot + pipeline_chunks - 1) / pipeline_chunks : ntot;
        if (chunk > want) chunk = want;
    }
    if (chunk < 1) return 0;
    if (chunk > ntot) chunk = ntot;
    if (chunk > 60000) chunk = 60000;    // grid.y limit of the J/K kernel
    return chunk;
}

bool defer_small_groups(const long* nfrag, const int* nao, int ngroups, long defer_min)
{
    auto weight = [&](int k) { const double n = (double)nao[k]; return (double)nfrag[k] * n * n * n * n; };
    bool defer = ngroups > 0 && defer_min > 0 && nfrag[0] >= defer_min;
    for (int k = 1; k < ngroups && defer; ++k) defer = 8.0 * weight(k) <= weight(0);
    return defer;
}

double nuclear_repulsion(const Topology& topo, const double* xyz)
{
    double e = 0.0;
    for (int i = 0; i < topo.natoms; ++i)
        for (int j = 0; j < i; ++j) {
            if (topo.zeff[i] == 0.0 || topo.zeff[j] == 0.0) continue;
            const double dx = xyz[3 * i] - xyz[3 * j], dy = xyz[3 * i + 1] - xyz[3 * j + 1], dz = xyz[3 * i + 2] - xyz[3 * j + 2];
            e += topo.zeff[i] * topo.zeff[j] / std::sqrt(dx * dx + dy * dy + dz * dz);
        }
    return e;
}

}  // namespace mqc

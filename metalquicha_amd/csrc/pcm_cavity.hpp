// pcm_cavity.hpp -- the solute cavity of the C-PCM (conductor-like polarisable continuum) stage: radii, the tesserae of
// one geometry, counts and the chunk stride.  Plain C++ (no HIP): whoever plans a batch uses it, and
// tests/host/check_pcm_cavity.cpp compiles it alone.
//
// Model: one sphere per real (non-ghost) atom I at R_I with radius rho_I = radius_scale x Bondi
// radius (or the caller's own table, in Bohr and unscaled); a Lebedev rule of angular_points directions u_k and weights
// w_k (sum w = 1) on every sphere gives the tesserae s = R_I + rho_I u_k with areas a = 4 pi rho_I^2 w_k; a tessera is
// KEPT iff |s - R_J| >= rho_J for every other real atom J (a sharp cut: energies only).  Order: by atom, then by the
// rule's own order.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>
#include "lebedev_tables.inc"

namespace mqc {
namespace pcm {

constexpr double ANGSTROM_TO_BOHR = 1.0 / 0.529177210903;   // CODATA 2018, as metalquicha_amd/basis.py
constexpr int MAX_TESSERAE = 4096;                           // per fragment
constexpr int MAX_ANGULAR_POINTS = 590;
constexpr int RADII_TABLE_LEN = 119;                         // a caller's radii_by_z: index = atomic number, 0..118
constexpr double ZETA = 4.90;                                // Gaussian blur of a tessera: zeta_i = ZETA / sqrt(a_i)

// Bondi radius in Angstrom, 0 where the table has none
inline double bondi_angstrom(int z)
{
    switch (z) {
        case 1: return 1.20; case 2: return 1.40; case 3: return 1.82; case 6: return 1.70; case 7: return 1.55;
        case 8: return 1.52; case 9: return 1.47; case 10: return 1.54; case 11: return 2.27; case 12: return 1.73;
        case 14: return 2.10; case 15: return 1.80; case 16: return 1.80; case 17: return 1.75; case 18: return 1.88;
        default: return 0.0;
    }
}

// index of the Lebedev rule with npts points among the rules the cavity may use, or -1
inline int rule_index(int npts)
{
    if (npts > MAX_ANGULAR_POINTS) return -1;
    for (int i = 0; i < LEBEDEV_NORDERS; ++i)
        if (LEBEDEV_ORDERS[i] == npts) return i;
    return -1;
}

// Sphere radius (Bohr) of every atom, 0 for a ghost.  radii_by_z (optional, RADII_TABLE_LEN entries, Bohr, unscaled)
// overrides the built-in value where it is non-zero.  false: an atom has no radius from either source (err names it).
inline bool sphere_radii(int natoms, const int* Z, const unsigned char* ghost, double radius_scale, const double* radii_by_z,
                         std::vector<double>& rho, std::string& err)
{
    rho.assign((size_t)natoms, 0.0);
    for (int a = 0; a < natoms; ++a) {
        if (ghost && ghost[a]) continue;
        const int z = Z[a];
        double r = 0.0;
        if (radii_by_z && z >= 0 && z < RADII_TABLE_LEN && radii_by_z[z] != 0.0) r = radii_by_z[z];
        else r = radius_scale * bondi_angstrom(z) * ANGSTROM_TO_BOHR;
        if (!(r > 0.0) || !std::isfinite(r)) {
            err = "PCM: no cavity radius for the element Z = " + std::to_string(z) + " (atom " + std::to_string(a) +
                  "): it is not in the built-in Bondi table and the caller's radii_by_z gives none";
            return false;
        }
        rho[(size_t)a] = r;
    }
    return true;
}

struct Cavity {
    int count = 0;                    // T, the tesserae kept
    std::vector<double> xyza;         // [T][4] = x, y, z (Bohr), area (Bohr^2)
    std::vector<int> atom;            // [T] the sphere a tessera sits on
    std::vector<int> per_atom;        // [natoms] tesserae kept on every sphere
};

// The tesserae of one geometry.  rho: sphere radii, 0 = no sphere (ghost).  false: an unknown rule or more than
// MAX_TESSERAE tesserae (err says which); the cavity then holds the count only.
inline bool build_cavity(int natoms, const double* xyz, const double* rho, int angular_points, Cavity& cav, std::string& err)
{
    cav = Cavity();
    cav.per_atom.assign((size_t)natoms, 0);
    const int ri = rule_index(angular_points);
    if (ri < 0) {
        err = "PCM: angular_points = " + std::to_string(angular_points) + " is not a Lebedev rule of the engine up to " +
              std::to_string(MAX_ANGULAR_POINTS) + " points (38, 50, 74, 86, 110, 146, 170, 194, 230, 266, 302, 350, 434, 590)";
        return false;
    }
    for (int a = 0; a < natoms; ++a) {
        const double ra = rho[a];
        if (!(ra > 0.0)) continue;
        for (int k = LEBEDEV_OFFSETS[ri]; k < LEBEDEV_OFFSETS[ri + 1]; ++k) {
            const double sx = xyz[3 * a] + ra * LEBEDEV_XYZW[k][0], sy = xyz[3 * a + 1] + ra * LEBEDEV_XYZW[k][1],
                         sz = xyz[3 * a + 2] + ra * LEBEDEV_XYZW[k][2];
            bool keep = true;
            for (int b = 0; b < natoms && keep; ++b) {
                if (b == a || !(rho[b] > 0.0)) continue;
                const double dx = sx - xyz[3 * b], dy = sy - xyz[3 * b + 1], dz = sz - xyz[3 * b + 2];
                keep = std::sqrt(dx * dx + dy * dy + dz * dz) >= rho[b];
            }
            if (!keep) continue;
            cav.xyza.push_back(sx); cav.xyza.push_back(sy); cav.xyza.push_back(sz);
            cav.xyza.push_back(4.0 * M_PI * ra * ra * LEBEDEV_XYZW[k][3]);
            cav.atom.push_back(a);
            cav.per_atom[(size_t)a] += 1;
            cav.count += 1;
        }
    }
    if (cav.count > MAX_TESSERAE) {
        err = "PCM: the cavity has " + std::to_string(cav.count) + " tesserae, above the limit of " + std::to_string(MAX_TESSERAE) +
              " per fragment; use fewer angular_points";
        cav.xyza.clear(); cav.atom.clear();
        return false;
    }
    return true;
}

// stride of the per-fragment PCM arrays of a chunk: the batch's largest tessera count rounded up to 64
inline int chunk_stride(int largest_count) { return largest_count <= 0 ? 0 : (largest_count + 63) / 64 * 64; }

}  // namespace pcm
}  // namespace mqc

// check_pcm_cavity.cpp -- stand-alone host check of metalquicha_amd/csrc/pcm_cavity.hpp (no HIP, no GPU): counts and
// areas against closed forms, ghosts, the tessera cap, radius overrides; `dump` prints a cavity for the comparison with
// the numpy reference (tests/test_pcm_cavity_host.py).
#include "../../metalquicha_amd/csrc/pcm_cavity.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mqc::pcm;

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } \
    } while (0)

static double total_area(const Cavity& c)
{
    double a = 0.0;
    for (int t = 0; t < c.count; ++t) a += c.xyza[4 * (size_t)t + 3];
    return a;
}

// dump numbers(+ghost flags) xyz: "Z g x y z" per atom on the command line after the rule
static int dump(int argc, char** argv)
{
    const int pts = std::atoi(argv[2]);
    const double scale = std::atof(argv[3]);
    const int natoms = (argc - 4) / 5;
    std::vector<int> z(natoms);
    std::vector<unsigned char> ghost(natoms);
    std::vector<double> xyz(3 * (size_t)natoms), rho;
    for (int a = 0; a < natoms; ++a) {
        z[a] = std::atoi(argv[4 + 5 * a]); ghost[a] = (unsigned char)std::atoi(argv[5 + 5 * a]);
        for (int c = 0; c < 3; ++c) xyz[3 * (size_t)a + c] = std::strtod(argv[6 + 5 * a + c], nullptr);
    }
    std::string err;
    if (!sphere_radii(natoms, z.data(), ghost.data(), scale, nullptr, rho, err)) { std::printf("error %s\n", err.c_str()); return 1; }
    Cavity cav;
    if (!build_cavity(natoms, xyz.data(), rho.data(), pts, cav, err)) { std::printf("error %s\n", err.c_str()); return 1; }
    std::printf("%d\n", cav.count);
    for (int t = 0; t < cav.count; ++t)
        std::printf("%d %.17g %.17g %.17g %.17g\n", cav.atom[t], cav.xyza[4 * (size_t)t], cav.xyza[4 * (size_t)t + 1], cav.xyza[4 * (size_t)t + 2],
                    cav.xyza[4 * (size_t)t + 3]);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && std::strcmp(argv[1], "dump") == 0) return dump(argc, argv);
    std::string err;
    std::vector<double> rho;
    Cavity cav;

    // (a) one sphere: every point of the rule, the whole area 4 pi rho^2, every tessera on the sphere
    {
        const int z[1] = {8};
        const double xyz[3] = {0.4, -1.1, 2.0};
        CHECK(sphere_radii(1, z, nullptr, 1.2, nullptr, rho, err), "%s", err.c_str());
        CHECK(std::fabs(rho[0] - 1.2 * 1.52 * ANGSTROM_TO_BOHR) < 1e-15, "oxygen radius %.17g", rho[0]);
        for (int pts : {38, 50, 110, 194, 302, 590}) {
            CHECK(build_cavity(1, xyz, rho.data(), pts, cav, err), "%s", err.c_str());
            CHECK(cav.count == pts, "one sphere, %d points: kept %d", pts, cav.count);
            const double full = 4.0 * M_PI * rho[0] * rho[0];
            CHECK(std::fabs(total_area(cav) - full) < 1e-12 * full, "one sphere, %d points: area %.15g vs %.15g", pts, total_area(cav), full);
            for (int t = 0; t < cav.count; ++t) {
                const double dx = cav.xyza[4 * (size_t)t] - xyz[0], dy = cav.xyza[4 * (size_t)t + 1] - xyz[1], dz = cav.xyza[4 * (size_t)t + 2] - xyz[2];
                CHECK(std::fabs(std::sqrt(dx * dx + dy * dy + dz * dz) - rho[0]) < 1e-13, "tessera %d off the sphere", t);
            }
        }
        std::printf("(a) one sphere: counts and areas ok\n");
    }
    // (b) two equal spheres at distance d: each loses the cap inside the other, of height h = rho - d/2 and area
    // 2 pi rho h; a Lebedev rule integrates the cap's indicator to a few tesserae's worth, and the two spheres keep the
    // same number by symmetry (the rules are inversion-symmetric and the axis is z)
    {
        const int z[2] = {6, 6};
        CHECK(sphere_radii(2, z, nullptr, 1.2, nullptr, rho, err), "%s", err.c_str());
        const double r = rho[0];
        for (double d : {0.5 * r, 1.0 * r, 1.5 * r, 2.5 * r}) {
            const double xyz[6] = {0, 0, 0, 0, 0, d};
            CHECK(build_cavity(2, xyz, rho.data(), 590, cav, err), "%s", err.c_str());
            const double h = d < 2 * r ? r - 0.5 * d : 0.0;
            const double exact = 2.0 * (4.0 * M_PI * r * r - 2.0 * M_PI * r * h);
            CHECK(cav.per_atom[0] == cav.per_atom[1], "two spheres at %.3f: %d and %d tesserae", d, cav.per_atom[0], cav.per_atom[1]);
            CHECK(cav.per_atom[0] + cav.per_atom[1] == cav.count, "per-atom counts do not add up");
            // the cut runs along one circle per sphere, of length at most 2 pi r: only the tesserae astride it can be
            // wrong, each by at most half its area a = 4 pi r^2 / N; there are (circle length) / sqrt(a) of them
            const double a = 4.0 * M_PI * r * r / 590.0;
            const double bound = 2.0 * (2.0 * M_PI * r / std::sqrt(a)) * 0.5 * a;
            CHECK(std::fabs(total_area(cav) - exact) <= bound, "two spheres at %.3f: area %.6f vs %.6f (bound %.6f)", d, total_area(cav), exact, bound);
            if (d >= 2 * r) CHECK(cav.count == 2 * 590, "disjoint spheres keep everything, kept %d", cav.count);
            for (int t = 0; t < cav.count; ++t) {
                const int other = 1 - cav.atom[t];
                const double dz = cav.xyza[4 * (size_t)t + 2] - xyz[3 * other + 2];
                const double dist = std::sqrt(cav.xyza[4 * (size_t)t] * cav.xyza[4 * (size_t)t] + cav.xyza[4 * (size_t)t + 1] * cav.xyza[4 * (size_t)t + 1] + dz * dz);
                CHECK(dist >= r, "a kept tessera lies inside the other sphere");
            }
        }
        std::printf("(b) two equal spheres: cap areas ok\n");
    }
    // (c) ghosts carry no sphere and cut nothing
    {
        const int z[3] = {8, 1, 1};
        const unsigned char ghost[3] = {0, 1, 1};
        const double xyz[9] = {0, 0, 0.19, 0, 1.46, -0.88, 0, -1.46, -0.88};
        CHECK(sphere_radii(3, z, ghost, 1.2, nullptr, rho, err), "%s", err.c_str());
        CHECK(rho[1] == 0.0 && rho[2] == 0.0 && rho[0] > 0.0, "ghost radii");
        CHECK(build_cavity(3, xyz, rho.data(), 110, cav, err), "%s", err.c_str());
        CHECK(cav.count == 110 && cav.per_atom[0] == 110 && cav.per_atom[1] == 0, "ghost hydrogens: kept %d", cav.count);
        CHECK(sphere_radii(3, z, nullptr, 1.2, nullptr, rho, err) && build_cavity(3, xyz, rho.data(), 110, cav, err), "%s", err.c_str());
        CHECK(cav.count < 330 && cav.per_atom[1] == cav.per_atom[2], "real hydrogens: kept %d", cav.count);
        std::printf("(c) ghosts ok\n");
    }
    // (d) the tessera cap and the rule table
    {
        std::vector<int> z(8, 18);
        std::vector<double> xyz;
        for (int a = 0; a < 8; ++a) { xyz.push_back(20.0 * a); xyz.push_back(0.0); xyz.push_back(0.0); }
        CHECK(sphere_radii(8, z.data(), nullptr, 1.2, nullptr, rho, err), "%s", err.c_str());
        CHECK(!build_cavity(8, xyz.data(), rho.data(), 590, cav, err), "8 x 590 tesserae must be refused");
        CHECK(cav.count == 8 * 590 && err.find("4096") != std::string::npos, "cap message: %s", err.c_str());
        CHECK(build_cavity(6, xyz.data(), rho.data(), 590, cav, err) && cav.count == 3540, "6 x 590 is legal");
        CHECK(!build_cavity(1, xyz.data(), rho.data(), 100, cav, err) && err.find("angular_points") != std::string::npos, "100 is no rule");
        CHECK(!build_cavity(1, xyz.data(), rho.data(), 770, cav, err), "770 is above the limit");
        CHECK(chunk_stride(163) == 192 && chunk_stride(64) == 64 && chunk_stride(65) == 128 && chunk_stride(0) == 0, "stride");
        std::printf("(d) cap, rules, stride ok\n");
    }
    // (e) radius overrides and missing radii
    {
        const int z[2] = {8, 26};
        std::vector<double> table(RADII_TABLE_LEN, 0.0);
        CHECK(!sphere_radii(2, z, nullptr, 1.2, nullptr, rho, err) && err.find("26") != std::string::npos, "iron has no Bondi radius: %s", err.c_str());
        table[26] = 3.7;
        CHECK(sphere_radii(2, z, nullptr, 1.2, table.data(), rho, err), "%s", err.c_str());
        CHECK(rho[1] == 3.7 && std::fabs(rho[0] - 1.2 * 1.52 * ANGSTROM_TO_BOHR) < 1e-15, "override is unscaled, zero means built-in");
        table[8] = 3.0;
        CHECK(sphere_radii(2, z, nullptr, 1.2, table.data(), rho, err) && rho[0] == 3.0, "oxygen override");
        const unsigned char ghost[2] = {0, 1};
        CHECK(sphere_radii(2, z, ghost, 1.2, nullptr, rho, err) && rho[1] == 0.0, "a ghost needs no radius");
        std::printf("(e) radii ok\n");
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}

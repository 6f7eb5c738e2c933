// cell_grid_host.cpp -- csrc/cell_grid.h on the host over adversarial inputs, built with -fsanitize=address,undefined and run
// as a program of its own (tests/test_cells_checker.py): pairs a hair closer than the length laid across cell walls, a
// lattice on the walls, coincident points, a clump between far outliers, coordinates of +-1e308, NaN and infinite points, no
// points at all.  Every world is checked for what the pair search rests on -- two gridded points with r2 < length * length,
// r2 formed as the kernels form it, have cell indices that differ by at most 1 on every axis -- and for in-range keys.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -I nbody-llm_amd/csrc tools/cell_grid_host.cpp
#include "cell_grid.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using nbody::cells::Grid;
using nbody::cells::kCellBits;
using nbody::cells::kCellMax;
using nbody::cells::kNoKey;

static unsigned long long g_state = 88172645463325252ull;
static double uniform01() {   // xorshift64
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return double(g_state >> 11) / 9007199254740992.0;
}

static long long axis_of(uint64_t key, int c) { return (long long)((key >> ((2 - c) * kCellBits)) & kCellMax); }

// returns the number of linked pairs; exits on a violation
static size_t check_world(const char* name, const std::vector<double>& xyz, double length, int want_usable) {
    const size_t n = xyz.size() / 3;
    std::vector<uint64_t> key(n + 1, 0x5a5a5a5a5a5a5a5aull);
    Grid g;
    const size_t n_gridded = nbody::cells::host_grid(xyz.data(), n, 3, length, &g, key.data());
    if (key[n] != 0x5a5a5a5a5a5a5a5aull) { std::printf("%s: wrote past the keys\n", name); std::exit(1); }
    if (want_usable >= 0 && g.usable != want_usable) { std::printf("%s: usable %d, want %d\n", name, g.usable, want_usable); std::exit(1); }
    size_t keyed = 0;
    for (size_t i = 0; i < n; ++i) keyed += key[i] != kNoKey;
    if (keyed != (g.usable ? n_gridded : 0)) { std::printf("%s: %zu keys for %zu gridded points\n", name, keyed, n_gridded); std::exit(1); }
    if (!g.usable) return 0;
    if (!(g.side > 0.0)) { std::printf("%s: side %g\n", name, g.side); std::exit(1); }
    const double B2 = length * length;
    size_t linked = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j) {
            const double dx = xyz[3 * j] - xyz[3 * i], dy = xyz[3 * j + 1] - xyz[3 * i + 1], dz = xyz[3 * j + 2] - xyz[3 * i + 2];
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            if (!(r2 < B2)) continue;
            ++linked;
            if (key[i] == kNoKey || key[j] == kNoKey) { std::printf("%s: pair (%zu, %zu) within the length is not gridded\n", name, i, j); std::exit(1); }
            for (int c = 0; c < 3; ++c)
                if (std::llabs(axis_of(key[i], c) - axis_of(key[j], c)) > 1) {
                    std::printf("%s: pair (%zu, %zu) within the length is no candidate pair on axis %d\n", name, i, j, c);
                    std::exit(1);
                }
        }
    return linked;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    size_t worlds = 0, linked = 0;
    const auto run = [&](const char* name, const std::vector<double>& xyz, double length, int want_usable) {
        linked += check_world(name, xyz, length, want_usable);
        ++worlds;
    };
    run("empty", {}, 1.0, 1);
    run("one", {1.0, 2.0, 3.0}, 0.5, 1);
    run("only nan", {nan, 0.0, 0.0, 0.0, inf, 0.0}, 0.5, 1);
    for (double b : {0.3, 1e-9, 1.0, 7.0e5, 1e-160, 4.9e-324, 1e150}) {
        // pairs a hair closer than b across the walls k * side, on each axis, at many places along the wall
        const double side = b * (1.0 + nbody::cells::kMargin);
        std::vector<double> xyz = {0.0, 0.0, 0.0};
        for (int axis = 0; axis < 3; ++axis)
            for (double sep : {std::nextafter(b, 0.0), b * (1.0 - 0x1p-50), b * 0.999})
                for (int k = 1; k < 40; k += 3)
                    for (double frac : {0.0, 0x1p-40, 0.25, 0.5, 1.0 - 0x1p-30, 1.0}) {
                        double a[3] = {7.0 * side, 7.0 * side, 7.0 * side};
                        a[(axis + 1) % 3] += 8.0 * double(xyz.size()) * side;
                        a[axis] = double(k) * side - frac * sep;
                        double c[3] = {a[0], a[1], a[2]};
                        c[axis] = a[axis] + sep;
                        xyz.insert(xyz.end(), a, a + 3);
                        xyz.insert(xyz.end(), c, c + 3);
                    }
        run("wall pairs", xyz, b, b * b < inf ? 1 : 0);
        // a lattice whose spacing is the side: every point on a wall
        std::vector<double> lat;
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) for (int k = 0; k < 5; ++k) { lat.push_back(i * side); lat.push_back(j * side); lat.push_back(k * side); }
        run("side lattice", lat, b, -1);
        run("side lattice, longer", lat, b * 1.75, -1);
    }
    {   // random clouds at several scales and offsets (lo != 0), lengths around the mean spacing
        for (double scale : {1.0, 1e-12, 1e9}) for (double off : {0.0, -3.7, 1e6}) {
            std::vector<double> xyz;
            for (int i = 0; i < 600; ++i) for (int c = 0; c < 3; ++c) xyz.push_back(off * scale + scale * uniform01());
            for (double b : {0.05, 0.11, 0.5}) run("cloud", xyz, b * scale, 1);
        }
    }
    {   // coincident points: E = 0
        std::vector<double> xyz;
        for (int i = 0; i < 50; ++i) { xyz.push_back(1.5); xyz.push_back(-2.25); xyz.push_back(0.75); }
        run("coincident", xyz, 1e-3, 1);
    }
    {   // a clump of width 4e-9 between outliers 1e3 apart, b = 1e-9: the side comes from E * 2^-20
        std::vector<double> xyz = {0.0, 0.0, 0.0, 1e3, 1e3, 1e3};
        for (int i = 0; i < 300; ++i) for (int c = 0; c < 3; ++c) xyz.push_back(1.0 + 4e-9 * uniform01());
        run("clump and outliers", xyz, 1e-9, 1);
        run("clump and outliers", xyz, 2.5e-9, 1);
    }
    {   // +-1e308: hi - lo overflows
        std::vector<double> xyz = {1e308, 0.0, 0.0, -1e308, 1.0, 0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.51};
        run("huge", xyz, 0.05, 0);
        run("huge, one sign", {1e308, 0.0, 0.0, 0.9e308, 0.0, 0.0, 0.5, 0.5, 0.5}, 1e300, 0);   // (length * length overflows)
        run("huge length", {0.0, 0.0, 0.0, 1.0, 1.0, 1.0}, 1.7e308, 0);
    }
    {   // NaN and infinite points among ordinary ones
        std::vector<double> xyz;
        for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) for (int k = 0; k < 5; ++k) { xyz.push_back(i); xyz.push_back(j); xyz.push_back(k); }
        xyz[3 * 7 + 2] = nan;
        xyz[3 * 9] = inf;
        xyz[3 * 11 + 1] = -inf;
        for (double b : {1.0, 1.001, 1.5}) run("holed lattice", xyz, b, 1);
    }
    std::printf("cell_grid_host ok: %zu worlds, %zu pairs within the length, all candidate pairs\n", worlds, linked);
    return 0;
}

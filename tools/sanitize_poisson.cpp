// sanitize_poisson.cpp -- the host side of the grid Poisson solve (nbody-llm_amd/csrc/poisson_grid.h: the tables, the transform,
// the check of a call and the whole of nbody_host_grid_poisson, which is host_entry there) under the host sanitizers: the refused
// calls, a 1x1x1 grid, lines along each axis alone, a periodic and an isolated cube, a point mass against 1 / r, the longest
// axis, in place, and the twiddle tables of every length.  A stand-alone program: build it on the CPU with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I nbody-llm_amd/csrc
//         tools/sanitize_poisson.cpp -o sanitize_poisson
// It prints "ok" only when every check held.
#include "poisson_grid.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace nbody::poisson;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

NbodyGridSpec spec_of(double spacing, int nx, int ny, int nz, int periodic, int scheme = NBODY_DEPOSIT_CIC, int axis = -1) {
    NbodyGridSpec s{};
    s.origin[0] = 3.0; s.origin[1] = -1e9; s.origin[2] = 0.5;   // ignored
    s.spacing = spacing;
    s.dims[0] = nx; s.dims[1] = ny; s.dims[2] = nz;
    s.scheme = scheme;
    s.quantity = 77;   // ignored
    s.periodic = periodic;
    s.project_axis = axis;
    return s;
}

NbodyPoissonSpec ps_of(double g, double soften = 0.0, int green = 0, int deconvolve = 0) {
    NbodyPoissonSpec p{};
    p.g = g;
    p.soften = soften;
    p.green = green;
    p.deconvolve = deconvolve;
    return p;
}

std::vector<double> ramp(size_t cells) {
    std::vector<double> m(cells);
    for (size_t i = 0; i < cells; ++i) m[i] = 1.0 + double((i * 7) % 13) * 0.125;
    return m;
}

bool all_finite(const std::vector<double>& v) {
    for (double x : v)
        if (!std::isfinite(x)) return false;
    return true;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

    // the refused calls: phi untouched
    {
        const std::vector<double> m = ramp(64);
        std::vector<double> phi(64, 7.0);
        const NbodyGridSpec ok = spec_of(0.5, 8, 4, 2, 0), per = spec_of(0.5, 8, 4, 2, 1);
        const NbodyPoissonSpec p = ps_of(1.0);
        CHECK(host_entry(nullptr, &p, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        CHECK(host_entry(&ok, nullptr, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        CHECK(host_entry(&ok, &p, nullptr, phi.data(), 64) == NBODY_ERR_INVALID);
        CHECK(host_entry(&ok, &p, m.data(), nullptr, 64) == NBODY_ERR_INVALID);
        CHECK(host_entry(&ok, &p, m.data(), phi.data(), 63) == NBODY_ERR_CAPACITY);
        const NbodyGridSpec bad_specs[] = {spec_of(0.0, 8, 4, 2, 0), spec_of(nan, 8, 4, 2, 0), spec_of(0.5, 6, 4, 2, 0), spec_of(0.5, 8, 4, 3, 1),
                                           spec_of(0.5, 0, 4, 2, 0), spec_of(0.5, 4096, 1, 1, 0), spec_of(0.5, 8192, 1, 1, 1),
                                           spec_of(0.5, 512, 512, 256, 0), spec_of(0.5, 1024, 1024, 256, 1), spec_of(0.5, 8, 4, 2, 0, 3),
                                           spec_of(0.5, 8, 4, 2, 0, NBODY_DEPOSIT_CIC, 0)};
        for (const NbodyGridSpec& s : bad_specs) CHECK(host_entry(&s, &p, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        const NbodyPoissonSpec bad_iso[] = {ps_of(nan), ps_of(inf), ps_of(1.0, nan), ps_of(1.0, inf), ps_of(1.0, -0.5), ps_of(1.0, 0.0, 1), ps_of(1.0, 0.0, 0, 1)};
        for (const NbodyPoissonSpec& b : bad_iso) CHECK(host_entry(&ok, &b, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        const NbodyPoissonSpec bad_per[] = {ps_of(1.0, 0.05), ps_of(1.0, 0.0, 2), ps_of(1.0, 0.0, -1), ps_of(1.0, 0.0, 0, 3), ps_of(1.0, 0.0, 0, -1)};
        for (const NbodyPoissonSpec& b : bad_per) CHECK(host_entry(&per, &b, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        NbodyPoissonSpec r = ps_of(1.0);
        r.reserved[1] = 1;
        CHECK(host_entry(&ok, &r, m.data(), phi.data(), 64) == NBODY_ERR_INVALID);
        for (double v : phi) CHECK(v == 7.0);
    }

    // a 1x1x1 grid: nothing is transformed; isolated and unsoftened it has no self term
    for (int periodic = 0; periodic < 2; ++periodic) {
        const NbodyGridSpec s = spec_of(0.5, 1, 1, 1, periodic);
        const NbodyPoissonSpec p = ps_of(1.0);
        const double m = 3.0;
        double phi = 7.0;
        CHECK(host_entry(&s, &p, &m, &phi, 1) == NBODY_OK);
        CHECK(phi == 0.0 && !std::signbit(phi));
    }

    // lines along each axis alone, both boundary conditions, every Green's function, deconvolution and scheme; column maps
    const int shapes[][3] = {{1, 1, 32}, {1, 32, 1}, {32, 1, 1}, {2, 2, 2}, {16, 8, 4}, {8, 8, 8}, {16, 16, 1}};
    for (const auto& d : shapes) {
        const size_t cells = size_t(d[0]) * size_t(d[1]) * size_t(d[2]);
        const std::vector<double> m = ramp(cells);
        for (int green = 0; green < 2; ++green)
            for (int dec = 0; dec < 3; ++dec)
                for (int scheme = 0; scheme < 3; ++scheme) {
                    const NbodyGridSpec s = spec_of(0.375, d[0], d[1], d[2], 1, scheme);
                    const NbodyPoissonSpec p = ps_of(1.25, 0.0, green, dec);
                    std::vector<double> phi(cells, 7.0);
                    CHECK(host_entry(&s, &p, m.data(), phi.data(), cells) == NBODY_OK);
                    CHECK(all_finite(phi));
                    double sum = 0.0, top = 0.0;
                    for (double v : phi) { sum += v; top = std::max(top, std::fabs(v)); }
                    CHECK(std::fabs(sum) <= 1e-12 * top * double(cells));   // the mean is removed
                }
        for (double soften : {0.0, 0.05}) {
            const NbodyGridSpec s = spec_of(0.375, d[0], d[1], d[2], 0, NBODY_DEPOSIT_TSC, d[2] == 1 ? 2 : -1);
            const NbodyPoissonSpec p = ps_of(1.25, soften);
            std::vector<double> phi(cells, 7.0);
            CHECK(host_entry(&s, &p, m.data(), phi.data(), cells) == NBODY_OK);
            CHECK(all_finite(phi));
            for (double v : phi) CHECK(v < 0.0);   // positive masses: an attractive potential everywhere
            std::vector<double> in_place = m;
            CHECK(host_entry(&s, &p, in_place.data(), in_place.data(), cells) == NBODY_OK);
            CHECK(in_place == phi);
        }
    }

    // a point mass on an isolated grid: phi = -g m / r at the other cells, +0.0 at its own
    {
        const NbodyGridSpec s = spec_of(0.5, 8, 8, 8, 0);
        const NbodyPoissonSpec p = ps_of(2.0);
        std::vector<double> m(512, 0.0), phi(512, 7.0);
        m[(size_t(1) * 8 + 2) * 8 + 3] = 4.0;
        CHECK(host_entry(&s, &p, m.data(), phi.data(), 512) == NBODY_OK);
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j)
                for (int l = 0; l < 8; ++l) {
                    const double dx = 0.5 * (i - 1), dy = 0.5 * (j - 2), dz = 0.5 * (l - 3), r = std::sqrt(dx * dx + dy * dy + dz * dz);
                    const double got = phi[(size_t(i) * 8 + size_t(j)) * 8 + size_t(l)];
                    if (r == 0.0) CHECK(std::fabs(got) <= 1e-13);
                    else CHECK(std::fabs(got + 8.0 / r) <= 1e-12 * (8.0 / r) + 1e-13);
                }
    }

    // an all-zero grid gives +0.0 everywhere
    for (int periodic = 0; periodic < 2; ++periodic) {
        const NbodyGridSpec s = spec_of(0.5, 8, 4, 2, periodic);
        const NbodyPoissonSpec p = ps_of(1.0);
        const std::vector<double> m(64, 0.0);
        std::vector<double> phi(64, 7.0);
        CHECK(host_entry(&s, &p, m.data(), phi.data(), 64) == NBODY_OK);
        for (double v : phi) CHECK(v == 0.0 && !std::signbit(v));
    }

    // the longest axis: 4096 periodic, 2048 padded to it
    {
        const std::vector<double> m = ramp(4096);
        std::vector<double> phi(4096, 7.0);
        const NbodyGridSpec a = spec_of(0.5, 4096, 1, 1, 1), b = spec_of(0.5, 1, 2, 2048, 0);
        const NbodyPoissonSpec pa = ps_of(1.0, 0.0, NBODY_POISSON_DIFF2, 2), pb = ps_of(1.0, 0.05);
        CHECK(host_entry(&a, &pa, m.data(), phi.data(), 4096) == NBODY_OK && all_finite(phi));
        CHECK(host_entry(&b, &pb, m.data(), phi.data(), 4096) == NBODY_OK && all_finite(phi));
    }

    // the twiddle tables: every length, the refused ones, unit modulus
    for (int L = 2; L <= NBODY_POISSON_MAX_AXIS; L *= 2) {
        std::vector<double> t(size_t(L), 7.0);
        CHECK(host_twiddles(L, t.data()) == NBODY_OK);
        CHECK(t[0] == 1.0 && t[1] == 0.0 && !std::signbit(t[1]));
        if (L >= 4) CHECK(t[size_t(L / 2)] == 0.0 && t[size_t(L / 2) + 1] == -1.0);
        for (int k = 0; k < L / 2; ++k) CHECK(std::fabs(t[2 * size_t(k)] * t[2 * size_t(k)] + t[2 * size_t(k) + 1] * t[2 * size_t(k) + 1] - 1.0) < 1e-15);
    }
    {
        double t[8];
        for (int L : {0, 1, 3, 12, 8192, -4}) CHECK(host_twiddles(L, t) == NBODY_ERR_INVALID);
        CHECK(host_twiddles(8, nullptr) == NBODY_ERR_INVALID);
    }

    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

// sanitize_pm.cpp -- the host side of the particle-mesh field (nbody-llm_amd/csrc/pm_grid.h: the check of a call and the whole of
// nbody_host_pm_field, which is host_entry there, over deposit_grid.h, poisson_grid.h and sample_grid.h) under the host sanitizers:
// the refused calls, no body, no point, one body, bodies off the grid and not finite, every scheme and gradient on periodic,
// isolated and column grids, the composition by hand, the all-zero grid and every NULL that is allowed.  A stand-alone program:
// build it on the CPU with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I nbody-llm_amd/csrc
//         tools/sanitize_pm.cpp -o sanitize_pm
// It prints "ok" only when every check held.
#include "pm_grid.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace nbody::pm;

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
    s.origin[0] = -2.0; s.origin[1] = -2.0; s.origin[2] = axis == 2 ? 0.0 : -2.0;
    s.spacing = spacing;
    s.dims[0] = nx; s.dims[1] = ny; s.dims[2] = nz;
    s.scheme = scheme;
    s.quantity = NBODY_DEPOSIT_MASS;
    s.periodic = periodic;
    s.project_axis = axis;
    return s;
}

NbodyPmSpec pm_of(double g, int gradient, double soften = 0.0, int green = 0, int deconvolve = 0) {
    NbodyPmSpec p{};
    p.poisson.g = g;
    p.poisson.soften = soften;
    p.poisson.green = green;
    p.poisson.deconvolve = deconvolve;
    p.gradient = gradient;
    return p;
}

// n bodies in and around [-2, 2]^3 with unequal masses, from a small generator of its own
void world(size_t n, std::vector<double>* xyz, std::vector<double>* m) {
    xyz->resize(3 * n);
    m->resize(n);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    auto next = [&s]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return double(s >> 11) / 9007199254740992.0;
    };
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) (*xyz)[3 * i + size_t(c)] = -2.6 + 5.2 * next();   // some of them off a grid that is not periodic
        (*m)[i] = (0.5 + next()) / double(n);
    }
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> xyz, m;
    world(257, &xyz, &m);
    xyz[3 * 7] = nan;          // one body that is not finite
    xyz[3 * 9 + 1] = 1.0e9;    // one far off every grid
    const size_t n = m.size();

    // the refused calls: nothing written
    {
        std::vector<double> acc(3 * n, 7.0), phi(n, 7.0);
        std::vector<uint8_t> cls(n, 9);
        uint64_t counts[8] = {99, 99, 99, 99, 99, 99, 99, 99};
        const NbodyGridSpec ok = spec_of(0.5, 8, 8, 8, 1);
        const NbodyPmSpec p = pm_of(1.0, NBODY_SAMPLE_GRADIENT2);
        auto call = [&](const NbodyGridSpec* s, const NbodyPmSpec* q) {
            return host_entry(xyz.data(), m.data(), n, s, q, nullptr, 0, acc.data(), phi.data(), cls.data(), counts);
        };
        CHECK(call(&ok, &p) == NBODY_OK);
        std::fill(acc.begin(), acc.end(), 7.0);
        std::fill(phi.begin(), phi.end(), 7.0);
        std::fill(cls.begin(), cls.end(), uint8_t(9));
        std::fill(counts, counts + 8, uint64_t(99));
        CHECK(call(nullptr, &p) == NBODY_ERR_INVALID);
        CHECK(call(&ok, nullptr) == NBODY_ERR_INVALID);
        NbodyGridSpec bad_specs[] = {spec_of(0.0, 8, 8, 8, 1), spec_of(nan, 8, 8, 8, 1), spec_of(0.5, 8, 6, 8, 1), spec_of(0.5, 0, 8, 8, 1),
                                     spec_of(0.5, 4096, 1, 1, 0), spec_of(0.5, 8, 8, 8, 1, 3), spec_of(0.5, 8, 8, 8, 1, NBODY_DEPOSIT_CIC, 0),
                                     spec_of(0.5, 8, 8, 8, 1), spec_of(0.5, 8, 8, 8, 1), spec_of(0.5, 8, 8, 8, 1)};
        bad_specs[7].quantity = NBODY_DEPOSIT_NUMBER;
        bad_specs[8].quantity = 6;
        bad_specs[9].reserved = 1;
        for (const NbodyGridSpec& s : bad_specs) CHECK(call(&s, &p) == NBODY_ERR_INVALID);
        NbodyPmSpec bad_pms[] = {pm_of(nan, 1), pm_of(inf, 1), pm_of(1.0, 1, 0.05), pm_of(1.0, 1, 0.0, 2), pm_of(1.0, 1, 0.0, 0, 3), pm_of(1.0, 0),
                                 pm_of(1.0, 3), pm_of(1.0, -1), pm_of(1.0, 1), pm_of(1.0, 1), pm_of(1.0, 1), pm_of(1.0, 1)};
        bad_pms[8].reserved[0] = 1;
        bad_pms[9].reserved[1] = 1;
        bad_pms[10].reserved[2] = 1;
        bad_pms[11].poisson.reserved[0] = 1;
        for (const NbodyPmSpec& q : bad_pms) CHECK(call(&ok, &q) == NBODY_ERR_INVALID);
        const NbodyGridSpec iso = spec_of(0.5, 8, 8, 8, 0);
        const NbodyPmSpec bad_iso[] = {pm_of(1.0, 1, -0.5), pm_of(1.0, 1, 0.0, 1), pm_of(1.0, 1, 0.0, 0, 1)};
        for (const NbodyPmSpec& q : bad_iso) CHECK(call(&iso, &q) == NBODY_ERR_INVALID);
        CHECK(host_entry(nullptr, m.data(), n, &ok, &p, nullptr, 0, acc.data(), nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        CHECK(host_entry(xyz.data(), nullptr, n, &ok, &p, nullptr, 0, acc.data(), nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        CHECK(host_entry(xyz.data(), m.data(), n, &ok, &p, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        CHECK(host_entry(xyz.data(), m.data(), size_t(1) << 31, &ok, &p, nullptr, 0, acc.data(), nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        CHECK(host_entry(xyz.data(), m.data(), n, &ok, &p, xyz.data(), size_t(1) << 31, acc.data(), nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        CHECK(host_entry(xyz.data(), m.data(), n, &ok, &p, xyz.data(), 2, nullptr, nullptr, nullptr, nullptr) == NBODY_ERR_INVALID);
        for (double v : acc) CHECK(v == 7.0);
        for (double v : phi) CHECK(v == 7.0);
        for (uint8_t v : cls) CHECK(v == 9);
        for (uint64_t v : counts) CHECK(v == 99);
    }

    // every scheme and gradient on a periodic, an isolated and a column grid, at the bodies and at points; the composition by hand
    const NbodyGridSpec grids[] = {spec_of(0.5, 8, 8, 8, 1), spec_of(0.25, 16, 8, 4, 1), spec_of(0.25, 8, 4, 2, 0), spec_of(0.25, 16, 16, 1, 0, 0, 2),
                                   spec_of(4.0, 1, 1, 1, 0), spec_of(4.0, 1, 1, 1, 1)};
    std::vector<double> pts(xyz.begin(), xyz.begin() + 3 * 40);
    pts[3 * 4 + 2] = inf;
    for (NbodyGridSpec s : grids)
        for (int scheme = 0; scheme < 3; ++scheme)
            for (int gradient = NBODY_SAMPLE_GRADIENT2; gradient <= NBODY_SAMPLE_GRADIENT4; ++gradient) {
                s.scheme = scheme;
                const NbodyPmSpec p = s.periodic ? pm_of(1.25, gradient, 0.0, gradient == 1 ? NBODY_POISSON_DIFF2 : NBODY_POISSON_SPECTRAL, gradient - 1)
                                                 : pm_of(1.25, gradient, gradient == 1 ? 0.0 : 0.05);
                const size_t cells = size_t(s.dims[0]) * size_t(s.dims[1]) * size_t(s.dims[2]);
                std::vector<double> grid(cells, 7.0);
                uint64_t c_dep[4], c_smp[4];
                CHECK(nbody::deposit::host_entry(xyz.data(), m.data(), n, &s, grid.data(), cells, c_dep) == NBODY_OK);
                CHECK(nbody::poisson::host_entry(&s, &p.poisson, grid.data(), grid.data(), cells) == NBODY_OK);
                for (int at_points = 0; at_points < 2; ++at_points) {
                    const double* P = at_points ? pts.data() : xyz.data();
                    const size_t np = at_points ? pts.size() / 3 : n;
                    std::vector<double> acc(3 * np, 7.0), phi(np, 7.0), grad(3 * np, 7.0), val(np, 7.0);
                    std::vector<uint8_t> cls(np, 9), cls_by_hand(np, 9);
                    uint64_t counts[8];
                    CHECK(host_entry(xyz.data(), m.data(), n, &s, &p, at_points ? P : nullptr, at_points ? np : 12345, acc.data(), phi.data(), cls.data(),
                                     counts) == NBODY_OK);
                    CHECK(nbody::sample::host_entry(P, np, &s, grid.data(), 1, gradient, grad.data(), cls_by_hand.data(), c_smp) == NBODY_OK);
                    CHECK(nbody::sample::host_entry(P, np, &s, grid.data(), 1, NBODY_SAMPLE_VALUE, val.data(), nullptr, nullptr) == NBODY_OK);
                    for (size_t i = 0; i < 3 * np; ++i) CHECK(std::memcmp(&acc[i], &(grad[i] = 0.0 - grad[i]), 8) == 0);
                    CHECK(std::memcmp(phi.data(), val.data(), 8 * np) == 0 && cls == cls_by_hand);
                    for (int k = 0; k < 4; ++k) CHECK(counts[k] == c_dep[k] && counts[4 + k] == c_smp[k]);
                    CHECK(counts[0] + counts[1] + counts[2] + counts[3] == n && counts[4] + counts[5] + counts[6] + counts[7] == np);
                    // phi, cls and counts NULL
                    std::vector<double> bare(3 * np, 7.0);
                    CHECK(host_entry(xyz.data(), m.data(), n, &s, &p, at_points ? P : nullptr, np, bare.data(), nullptr, nullptr, nullptr) == NBODY_OK);
                    CHECK(bare == acc || std::memcmp(bare.data(), acc.data(), 24 * np) == 0);
                }
                // no body (every output +0.0), no point, one body
                {
                    std::vector<double> acc(3 * 40, 7.0), phi(40, 7.0);
                    uint64_t counts[8];
                    CHECK(host_entry(nullptr, nullptr, 0, &s, &p, pts.data(), 40, acc.data(), phi.data(), nullptr, counts) == NBODY_OK);
                    for (double v : acc) CHECK(v == 0.0 && !std::signbit(v));
                    for (double v : phi) CHECK(v == 0.0 && !std::signbit(v));
                    CHECK(counts[0] + counts[1] + counts[2] + counts[3] == 0);
                    CHECK(host_entry(nullptr, nullptr, 0, &s, &p, nullptr, 0, nullptr, nullptr, nullptr, counts) == NBODY_OK);
                    CHECK(host_entry(xyz.data(), m.data(), n, &s, &p, pts.data(), 0, nullptr, nullptr, nullptr, counts) == NBODY_OK);
                    CHECK(counts[0] + counts[1] + counts[2] + counts[3] == n && counts[4] + counts[5] + counts[6] + counts[7] == 0);
                    CHECK(host_entry(xyz.data(), m.data(), 1, &s, &p, nullptr, 0, acc.data(), phi.data(), nullptr, counts) == NBODY_OK);
                    CHECK(std::isfinite(acc[0]) && std::isfinite(phi[0]));
                }
                // massless bodies: an all-zero grid, +0.0 everywhere
                {
                    const std::vector<double> zero(n, 0.0);
                    std::vector<double> acc(3 * n, 7.0), phi(n, 7.0);
                    CHECK(host_entry(xyz.data(), zero.data(), n, &s, &p, nullptr, 0, acc.data(), phi.data(), nullptr, nullptr) == NBODY_OK);
                    for (double v : acc) CHECK(v == 0.0 && !std::signbit(v));
                    for (double v : phi) CHECK(v == 0.0 && !std::signbit(v));
                }
            }

    if (g_failed) {
        std::printf("%d checks failed\n", g_failed);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}

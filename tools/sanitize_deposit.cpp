// sanitize_deposit.cpp -- the host side of the grid deposit (nbody-llm_amd/csrc/deposit_grid.h: the stencils, the index
// arithmetic, the check of a spec and the whole of nbody_host_deposit, which is host_entry there) under the host sanitizers:
// empty inputs, a 1x1x1 grid, periodic wrap with bodies thousands of periods away, the edges of |u| < 2^31, and grids at the
// cell limit in the index arithmetic.  A stand-alone program: build it on the CPU with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I nbody-llm_amd/csrc
//         tools/sanitize_deposit.cpp -o sanitize_deposit
// It prints "ok" only when every check held.
#include "deposit_grid.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace nbody::deposit;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

NbodyGridSpec spec_of(double ox, double oy, double oz, double spacing, int nx, int ny, int nz, int scheme, int periodic = 0, int axis = -1) {
    NbodyGridSpec s{};
    s.origin[0] = ox; s.origin[1] = oy; s.origin[2] = oz;
    s.spacing = spacing;
    s.dims[0] = nx; s.dims[1] = ny; s.dims[2] = nz;
    s.scheme = scheme;
    s.quantity = NBODY_DEPOSIT_MASS;
    s.periodic = periodic;
    s.project_axis = axis;
    return s;
}

double sum_of(const std::vector<double>& g) {
    double s = 0.0;
    for (double v : g) s += v;
    return s;
}

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t counts[4];

    // empty inputs: no body, NULL arrays; every cell +0.0
    for (int scheme = 0; scheme < 3; ++scheme) {
        const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 3, 2, 1, scheme);
        std::vector<double> grid(6, 7.0);
        CHECK(host_entry(nullptr, nullptr, 0, &s, grid.data(), grid.size(), counts) == NBODY_OK);
        for (double v : grid) CHECK(v == 0.0 && !std::signbit(v));
        CHECK(counts[0] + counts[1] + counts[2] + counts[3] == 0);
        CHECK(host_entry(nullptr, nullptr, 0, &s, nullptr, 0, counts) == NBODY_OK);
        CHECK(host_entry(nullptr, nullptr, 1, &s, grid.data(), grid.size(), counts) == NBODY_ERR_INVALID);
        CHECK(host_entry(nullptr, nullptr, 0, &s, grid.data(), 5, counts) == NBODY_ERR_CAPACITY);
        CHECK(host_entry(nullptr, nullptr, 0, nullptr, grid.data(), 6, counts) == NBODY_ERR_INVALID);
    }

    // a 1x1x1 grid: every scheme, with and without wrap; periodic: the whole of q lands in the one cell
    {
        const double xyz[] = {0.5, 0.5, 0.5, 0.01, 0.99, 0.5, -3.0, 9.0, 0.25, 1.0, 1.0, 1.0};
        const double q[] = {1.0, 0.5, 0.25, 2.0};
        for (int scheme = 0; scheme < 3; ++scheme)
            for (int periodic = 0; periodic < 2; ++periodic) {
                const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 1, 1, 1, scheme, periodic);
                std::vector<double> grid(1, -1.0);
                CHECK(host_entry(xyz, q, 4, &s, grid.data(), 1, counts) == NBODY_OK);
                CHECK(counts[0] + counts[1] + counts[2] + counts[3] == 4);
                if (periodic) CHECK(counts[0] == 4 && std::fabs(grid[0] - 3.75) < 1e-12);
                else CHECK(grid[0] > 0.0 && grid[0] <= 1.5 + 1e-12);
            }
    }

    // periodic wrap with bodies thousands of periods away on either side, and the edges of |u| < 2^31
    {
        std::vector<double> xyz, q;
        for (int k = -3000; k <= 3000; k += 250) {
            xyz.insert(xyz.end(), {0.3 + 4.0 * k, 1.7 - 4.0 * k, 3.999 + 4.0 * k});
            q.push_back(1.0 + 0.001 * k);
        }
        const size_t n_far = q.size();
        const double edge = 2147483648.0;   // u = 2^31 exactly: skipped; the double below it: the last index that is used
        xyz.insert(xyz.end(), {edge, 0.0, 0.0});                                  q.push_back(1.0);
        xyz.insert(xyz.end(), {std::nextafter(edge, 0.0), 0.0, 0.0});             q.push_back(1.0);
        xyz.insert(xyz.end(), {-edge, 0.0, 0.0});                                 q.push_back(1.0);
        xyz.insert(xyz.end(), {std::nextafter(-edge, 0.0), 0.0, 0.0});            q.push_back(1.0);
        xyz.insert(xyz.end(), {1e300, 0.0, 0.0});                                 q.push_back(1.0);
        xyz.insert(xyz.end(), {nan, 0.0, 0.0});                                   q.push_back(1.0);
        xyz.insert(xyz.end(), {0.0, inf, 0.0});                                   q.push_back(1.0);
        xyz.insert(xyz.end(), {0.0, 0.0, 0.0});                                   q.push_back(nan);
        for (int scheme = 0; scheme < 3; ++scheme)
            for (int periodic = 0; periodic < 2; ++periodic) {
                const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 4, 4, 4, scheme, periodic);
                std::vector<double> grid(64, 0.0);
                CHECK(host_entry(xyz.data(), q.data(), q.size(), &s, grid.data(), 64, counts) == NBODY_OK);
                CHECK(counts[3] == 6);   // 2^31, -2^31, 1e300, NaN, inf, NaN q
                CHECK(counts[0] + counts[1] + counts[2] + counts[3] == q.size());
                if (periodic) {
                    CHECK(counts[1] == 0 && counts[2] == 0);
                    double want = 2.0;   // the two bodies just inside the limit
                    for (size_t i = 0; i < n_far; ++i) want += q[i];
                    CHECK(std::fabs(sum_of(grid) - want) < 1e-9);
                }
            }
        // a column map ignores its axis altogether: a huge z is fine there, a NaN z is still skipped
        const double col[] = {0.5, 0.5, 1e300, 0.5, 0.5, nan};
        const double cq[] = {1.0, 1.0};
        const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 2, 2, 1, NBODY_DEPOSIT_TSC, 0, 2);
        std::vector<double> grid(4, 0.0);
        CHECK(host_entry(col, cq, 2, &s, grid.data(), 4, counts) == NBODY_OK);
        CHECK(counts[3] == 1 && counts[0] + counts[1] == 1);
    }

    // grids at the cell limit: the linear index of the last cell, dims whose product is exactly 2^27, one more is refused
    {
        const int shapes[][3] = {{134217728, 1, 1}, {1, 134217728, 1}, {1, 1, 134217728}, {512, 512, 512}, {1024, 1024, 128}, {2, 67108864, 1}};
        for (const auto& d : shapes) {
            const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, d[0], d[1], d[2], NBODY_DEPOSIT_CIC);
            CHECK(spec_refusal(&s, true).empty());
            const Grid g = grid_of(s);
            CHECK(cells_of(g) == size_t(NBODY_DEPOSIT_MAX_CELLS));
            // a body in the middle of the last cell: NGP's home cell is the last linear index
            NbodyGridSpec ngp = s;
            ngp.scheme = NBODY_DEPOSIT_NGP;
            Stencil st;
            CHECK(body_stencil(grid_of(ngp), d[0] - 0.5, d[1] - 0.5, d[2] - 0.5, 1.0, &st));
            CHECK(home_cell(grid_of(ngp), st) == uint32_t(NBODY_DEPOSIT_MAX_CELLS - 1));
            CHECK(body_class(st) == kInside);
            // counts only (grid == NULL): no 1 GiB array here
            const double xyz[] = {d[0] - 0.5, d[1] - 0.5, d[2] - 0.5, -0.25, -0.25, -0.25};
            const double q[] = {1.0, 1.0};
            CHECK(host_entry(xyz, q, 2, &s, nullptr, 0, counts) == NBODY_OK);
            CHECK(counts[1] == 2);   // CIC from the middle of a corner cell reaches off the grid on some axis
        }
        NbodyGridSpec over = spec_of(0, 0, 0, 1.0, 1024, 1024, 129, NBODY_DEPOSIT_NGP);
        CHECK(!spec_refusal(&over, true).empty());
        over = spec_of(0, 0, 0, 1.0, 2147483647, 2147483647, 2147483647, NBODY_DEPOSIT_NGP);
        CHECK(!spec_refusal(&over, true).empty());
        // a long thin grid that is deposited for real: the last cells of 2^20 x 1 x 1, wrapped from far below
        const NbodyGridSpec thin = spec_of(0, 0, 0, 1.0, 1 << 20, 1, 1, NBODY_DEPOSIT_TSC, 1);
        std::vector<double> grid(size_t(1) << 20, 0.0);
        const double xyz[] = {-0.5, 0.5, 0.5, double(1 << 20) * 2000.0 - 0.5, 0.5, 0.5};
        const double q[] = {1.0, 1.0};
        CHECK(host_entry(xyz, q, 2, &thin, grid.data(), grid.size(), counts) == NBODY_OK);
        CHECK(counts[0] == 2 && grid[(size_t(1) << 20) - 1] > 1.0 && std::fabs(sum_of(grid) - 2.0) < 1e-12);
    }

    // the scale: exponents of subnormal, tiny and huge q; S keeps ldexp in range and the sums in int64
    {
        CHECK(frexp_exponent(0.0) == 0 && frexp_exponent(1.0) == 1 && frexp_exponent(0.75) == 0 && frexp_exponent(4.9e-324) == -1073);
        CHECK(frexp_exponent(std::numeric_limits<double>::max()) == 1024);
        CHECK(ceil_log2(1) == 0 && ceil_log2(2) == 1 && ceil_log2(3) == 2 && ceil_log2(4099) == 13 && ceil_log2(0x7fffffffull) == 31);
        const double xyz[] = {0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5};
        for (double big : {4.9e-324, 1e-300, 1.0, 1e300, std::numeric_limits<double>::max()}) {
            const double q[] = {big, -big, big};
            const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 1, 1, 1, NBODY_DEPOSIT_NGP);
            double cell = 0.0;
            CHECK(host_entry(xyz, q, 3, &s, &cell, 1, counts) == NBODY_OK);
            CHECK(cell == big);
        }
    }

    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}

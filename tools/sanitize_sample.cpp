// sanitize_sample.cpp -- the host side of the grid sample (nbody-llm_amd/csrc/sample_grid.h: the differences, the index
// arithmetic, the check of a call and the whole of nbody_host_grid_sample, which is host_entry there) under the host sanitizers:
// empty inputs, a 1x1x1 grid, wraps from thousands of periods away, |u| at 2^31, gradients on axes of 1 to 4 cells periodic and
// not, and fields times cells exactly at the limit.  A stand-alone program: build it on the CPU with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I nbody-llm_amd/csrc
//         tools/sanitize_sample.cpp -o sanitize_sample
// It prints "ok" only when every check held.
#include "sample_grid.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace nbody::sample;

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
    s.quantity = 77;   // ignored
    s.periodic = periodic;
    s.project_axis = axis;
    return s;
}

// cells that are all different and exact: G[f][c] = c + 1000 f
std::vector<double> ramp(size_t cells, int fields = 1) {
    std::vector<double> g(cells * size_t(fields));
    for (size_t i = 0; i < g.size(); ++i) g[i] = double(i % cells) + 1000.0 * double(i / cells);
    return g;
}

const int kOps[3] = {NBODY_SAMPLE_VALUE, NBODY_SAMPLE_GRADIENT2, NBODY_SAMPLE_GRADIENT4};

}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t counts[4];

    // empty inputs: no point, NULL arrays; the refusals of a call
    for (int scheme = 0; scheme < 3; ++scheme)
        for (int op : kOps) {
            const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 3, 2, 1, scheme);
            const std::vector<double> grid = ramp(6);
            counts[0] = counts[1] = counts[2] = counts[3] = 9;
            CHECK(host_entry(nullptr, 0, &s, grid.data(), 1, op, nullptr, nullptr, counts) == NBODY_OK);
            CHECK(counts[0] + counts[1] + counts[2] + counts[3] == 0);
            CHECK(host_entry(nullptr, 0, &s, grid.data(), 1, op, nullptr, nullptr, nullptr) == NBODY_OK);
            double out[3];
            const double p[3] = {0.5, 0.5, 0.5};
            CHECK(host_entry(nullptr, 1, &s, grid.data(), 1, op, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, grid.data(), 1, op, nullptr, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, nullptr, 1, op, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, nullptr, grid.data(), 1, op, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, grid.data(), 0, op, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, grid.data(), 5, op, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, grid.data(), 1, 3, out, nullptr, counts) == NBODY_ERR_INVALID);
            CHECK(host_entry(p, 1, &s, grid.data(), 1, -1, out, nullptr, counts) == NBODY_ERR_INVALID);
            if (op != NBODY_SAMPLE_VALUE) CHECK(host_entry(p, 1, &s, grid.data(), 2, op, out, nullptr, counts) == NBODY_ERR_INVALID);
        }

    // a 1x1x1 grid: every scheme and op, with and without wrap; periodic: the value is the cell's, every gradient exactly +0.0
    {
        const double xyz[] = {0.5, 0.5, 0.5, 0.01, 0.99, 0.5, -3.0, 9.0, 0.25, 1.0, 1.0, 1.0};
        const double cell[4] = {2.5, -1.0, 4.0, 8.0};
        for (int scheme = 0; scheme < 3; ++scheme)
            for (int periodic = 0; periodic < 2; ++periodic)
                for (int op : kOps) {
                    const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 1, 1, 1, scheme, periodic);
                    const int fields = op == NBODY_SAMPLE_VALUE ? 4 : 1;
                    double out[4 * 4];
                    uint8_t cls[4];
                    CHECK(host_entry(xyz, 4, &s, cell, fields, op, out, cls, counts) == NBODY_OK);
                    CHECK(counts[0] + counts[1] + counts[2] + counts[3] == 4);
                    if (periodic) CHECK(counts[0] == 4);
                    for (int i = 0; i < 4; ++i)
                        for (int k = 0; k < width_of(op, fields); ++k) {
                            const double v = out[i * width_of(op, fields) + k];
                            if (op != NBODY_SAMPLE_VALUE) CHECK(v == 0.0 && !std::signbit(v));
                            else if (periodic) CHECK(std::fabs(v - cell[k]) < 1e-12);
                        }
                }
    }

    // wraps from thousands of periods away on either side, and the edges of |u| < 2^31
    {
        std::vector<double> xyz;
        for (int k = -3000; k <= 3000; k += 250) xyz.insert(xyz.end(), {0.3 + 4.0 * k, 1.7 - 4.0 * k, 3.999 + 4.0 * k});
        const size_t n_far = xyz.size() / 3;
        const double edge = 2147483648.0;   // u = 2^31 exactly: skipped; the double below it: the last index that is used
        xyz.insert(xyz.end(), {edge, 0.0, 0.0});
        xyz.insert(xyz.end(), {std::nextafter(edge, 0.0), 0.0, 0.0});
        xyz.insert(xyz.end(), {-edge, 0.0, 0.0});
        xyz.insert(xyz.end(), {std::nextafter(-edge, 0.0), 0.0, 0.0});
        xyz.insert(xyz.end(), {1e300, 0.0, 0.0});
        xyz.insert(xyz.end(), {nan, 0.0, 0.0});
        xyz.insert(xyz.end(), {0.0, inf, 0.0});
        const size_t n = xyz.size() / 3;
        const std::vector<double> grid = ramp(64);
        for (int scheme = 0; scheme < 3; ++scheme)
            for (int periodic = 0; periodic < 2; ++periodic)
                for (int op : kOps) {
                    const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 4, 4, 4, scheme, periodic);
                    std::vector<double> out(n * 3, -1.0);
                    std::vector<uint8_t> cls(n, 9);
                    CHECK(host_entry(xyz.data(), n, &s, grid.data(), 1, op, out.data(), cls.data(), counts) == NBODY_OK);
                    CHECK(counts[3] == 5);   // 2^31, -2^31, 1e300, NaN, inf
                    CHECK(counts[0] + counts[1] + counts[2] + counts[3] == n);
                    if (periodic) {
                        CHECK(counts[1] == 0 && counts[2] == 0);
                        if (op == NBODY_SAMPLE_VALUE)
                            for (size_t i = 0; i < n_far; ++i) CHECK(out[i] >= 0.0 && out[i] <= 63.0 * (1.0 + 1e-12));
                    }
                    for (size_t i = 0; i < n; ++i)
                        if (cls[i] == kSkipped || cls[i] == kOutside)
                            for (int k = 0; k < width_of(op, 1); ++k) CHECK(out[i * size_t(width_of(op, 1)) + k] == 0.0);
                }
        // a column map ignores its axis altogether: a huge z is fine there, a NaN z is still skipped; its component is +0.0
        const double col[] = {0.5, 0.5, 1e300, 0.5, 0.5, nan};
        const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, 2, 2, 1, NBODY_DEPOSIT_TSC, 1, 2);
        const std::vector<double> g4 = ramp(4);
        double out[6];
        uint8_t cls[2];
        CHECK(host_entry(col, 2, &s, g4.data(), 1, NBODY_SAMPLE_GRADIENT2, out, cls, counts) == NBODY_OK);
        CHECK(counts[3] == 1 && counts[0] == 1 && cls[1] == kSkipped && out[2] == 0.0 && !std::signbit(out[2]));
    }

    // gradients on axes of 1 to 4 cells, periodic and not: every neighbour index stays on the grid or the term is dropped
    {
        std::vector<double> xyz;
        for (double x = -1.25; x <= 5.25; x += 0.25)
            for (double y : {-0.5, 0.5, 1.75, 3.9}) xyz.insert(xyz.end(), {x, y, 0.5 * x + 0.125});
        const size_t n = xyz.size() / 3;
        for (int nx = 1; nx <= 4; ++nx)
            for (int ny = 1; ny <= 4; ++ny)
                for (int scheme = 0; scheme < 3; ++scheme)
                    for (int periodic = 0; periodic < 2; ++periodic)
                        for (int op : kOps) {
                            const int nz = 5 - nx;
                            const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, nx, ny, nz, scheme, periodic);
                            const std::vector<double> grid = ramp(size_t(nx) * size_t(ny) * size_t(nz));
                            std::vector<double> out(n * 3, -1.0);
                            std::vector<uint8_t> cls(n, 9);
                            CHECK(host_entry(xyz.data(), n, &s, grid.data(), 1, op, out.data(), cls.data(), counts) == NBODY_OK);
                            CHECK(counts[0] + counts[1] + counts[2] + counts[3] == n && counts[3] == 0);
                            if (op == NBODY_SAMPLE_VALUE) continue;
                            const int reach = reach_of(op);
                            const int dims[3] = {nx, ny, nz};
                            for (size_t i = 0; i < n; ++i)
                                for (int k = 0; k < 3; ++k) {
                                    const double v = out[3 * i + size_t(k)];
                                    // not periodic: an axis shorter than 2 reach + 1 cells holds no difference; periodic: an axis of
                                    // 1 or 2 cells gives exact zeros of order 2 (its two neighbours are one cell)
                                    if (!periodic && dims[k] < 2 * reach + 1) CHECK(v == 0.0 && !std::signbit(v));
                                    if (periodic && op == NBODY_SAMPLE_GRADIENT2 && dims[k] <= 2) CHECK(v == 0.0 && !std::signbit(v));
                                    if (periodic && dims[k] == 1) CHECK(v == 0.0 && !std::signbit(v));
                                }
                            if (!periodic && (nx < 2 * reach + 1 || ny < 2 * reach + 1 || nz < 2 * reach + 1)) CHECK(counts[0] == 0);
                        }
    }

    // fields times cells exactly at the limit: the check of a call, the linear index of the last cell of the last field
    {
        const int shapes[][4] = {{134217728, 1, 1, 1}, {1, 1, 134217728, 1}, {512, 512, 512, 1}, {1024, 1024, 32, 4}, {512, 512, 256, 2}, {2, 16777216, 1, 4}};
        const double one = 1.0;   // (stands for a grid that no point reads: n == 0)
        for (const auto& d : shapes) {
            const NbodyGridSpec s = spec_of(0, 0, 0, 1.0, d[0], d[1], d[2], NBODY_DEPOSIT_CIC);
            CHECK(call_refusal(&s, &one, d[3], NBODY_SAMPLE_VALUE).empty());
            CHECK(size_t(d[3]) * nbody::deposit::cells_of(nbody::deposit::grid_of(s)) == size_t(NBODY_DEPOSIT_MAX_CELLS));
            if (d[3] < 4) CHECK(!call_refusal(&s, &one, d[3] + 1, NBODY_SAMPLE_VALUE).empty());
            CHECK(host_entry(nullptr, 0, &s, &one, d[3], NBODY_SAMPLE_VALUE, nullptr, nullptr, counts) == NBODY_OK);
            const Grid g = nbody::deposit::grid_of(s);
            CHECK(linear_cell(g, d[0] - 1, d[1] - 1, d[2] - 1) + size_t(d[3] - 1) * nbody::deposit::cells_of(g) == size_t(NBODY_DEPOSIT_MAX_CELLS) - 1);
        }
        NbodyGridSpec over = spec_of(0, 0, 0, 1.0, 1024, 1024, 129, NBODY_DEPOSIT_NGP);
        CHECK(!call_refusal(&over, &one, 1, NBODY_SAMPLE_VALUE).empty());
        // a long thin grid that is sampled for real: the last cells of 2^20 x 1 x 1 x 4 fields, wrapped from far below, order 4
        const NbodyGridSpec thin = spec_of(0, 0, 0, 1.0, 1 << 20, 1, 1, NBODY_DEPOSIT_TSC, 1);
        const std::vector<double> grid = ramp(size_t(1) << 20, 4);
        const double xyz[] = {-0.5, 0.5, 0.5, double(1 << 20) * 2000.0 - 0.5, 0.5, 0.5, 0.5, 0.5, 0.5};
        double out[12];
        uint8_t cls[3];
        CHECK(host_entry(xyz, 3, &thin, grid.data(), 4, NBODY_SAMPLE_VALUE, out, cls, counts) == NBODY_OK);
        CHECK(counts[0] == 3 && out[0] == out[4] && out[3] == out[0] + 3000.0);
        CHECK(host_entry(xyz, 3, &thin, grid.data(), 1, NBODY_SAMPLE_GRADIENT4, out, cls, counts) == NBODY_OK);
        CHECK(counts[0] == 3 && out[1] == 0.0 && out[2] == 0.0 && out[0] == out[3] && out[0] < 0.0);
    }

    if (g_failed) return 1;
    std::printf("ok\n");
    return 0;
}

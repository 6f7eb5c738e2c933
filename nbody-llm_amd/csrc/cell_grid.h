// cell_grid.h -- the uniform cell grid of the fixed-radius pair search (include/nbody_hip.h, "pair search"), stated once: the
// kernels (kernels_cells.hip), the host side of a call (nbody_cells.cpp) and nbody_host_cell_grid all evaluate these functions,
// and tools/cell_grid_host.cpp drives them under the host sanitizers.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off.  All of it is f64 and every operation
// is rounded on its own, so the device, the host and the numpy restatement (tests/cells_ref.py) give the same bits:
//     GRIDDED        a body whose three coordinates are finite
//     lo_c, hi_c     min and max of the gridded bodies' coordinate c (exact; a zero bound is taken as +0.0)
//     E              max_c (hi_c - lo_c)
//     side           max(length * (1 + 2^-20), E * 2^-20)
//     k_c            min((uint64) floor((x_c - lo_c) / side), 2^21 - 1)
//     key            k_x << 42 | k_y << 21 | k_z          (ungridded bodies: all ones)
//     usable         isfinite(E) && isfinite(side) && isfinite(length * length)
// DESIGN 3.19 proves what the search rests on: two gridded bodies with r2 < fl(length * length) in the calls' own rounded
// arithmetic have cell indices that differ by at most 1 on every axis.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CELLS_HD __host__ __device__ inline
#else
#define CELLS_HD inline
#endif

namespace nbody { namespace cells {

constexpr int kCellBits = 21;                                   // bits of one axis in a key
constexpr uint64_t kCellMax = (uint64_t(1) << kCellBits) - 1;   // the highest cell index of an axis
constexpr uint64_t kNoKey = ~uint64_t(0);                       // the key of a body that is not gridded
constexpr double kMargin = 1.0 / 1048576.0;                     // 2^-20: of the side over the length, and cells per extent

struct Grid {
    double lo[3];
    double side;
    int usable;
};

CELLS_HD bool finite64(double v) { return v - v == 0.0; }   // (false for NaN and for either infinity)

CELLS_HD bool gridded(double x, double y, double z) { return finite64(x) && finite64(y) && finite64(z); }

// the grid of gridded bodies within [lo, hi] (any = false: of none -- lo = 0, E = 0) for the length of the call
CELLS_HD Grid make_grid(const double lo[3], const double hi[3], bool any, double length) {
    Grid g;
    double extent = 0.0;
    for (int c = 0; c < 3; ++c) {
        g.lo[c] = any ? lo[c] + 0.0 : 0.0;   // (-0.0 + 0.0 == +0.0)
        const double e = any ? hi[c] - lo[c] : 0.0;
        if (e > extent || e != e) extent = e;   // (no NaN arises from finite bounds; +inf does, by overflow)
    }
    const double by_length = length * (1.0 + kMargin), by_extent = extent * kMargin;
    g.side = by_length > by_extent ? by_length : by_extent;
    g.usable = finite64(extent) && finite64(g.side) && finite64(length * length);
    return g;
}

// the cell of coordinate x (gridded: lo <= x <= hi) along one axis of a usable grid
CELLS_HD uint64_t cell_index(double x, double lo, double side) {
    const double q = std::floor((x - lo) / side);
    return q >= double(kCellMax) ? kCellMax : uint64_t(q);   // (q >= 0: x >= lo and side > 0)
}

CELLS_HD uint64_t cell_key(uint64_t kx, uint64_t ky, uint64_t kz) { return kx << (2 * kCellBits) | ky << kCellBits | kz; }

CELLS_HD uint64_t body_key(const Grid& g, double x, double y, double z) {
    if (!gridded(x, y, z)) return kNoKey;
    return cell_key(cell_index(x, g.lo[0], g.side), cell_index(y, g.lo[1], g.side), cell_index(z, g.lo[2], g.side));
}

// ---- what the host needs of the whole computation: the bounds of n points {x, y, z} of `stride` doubles each (exact, in any
// order), the grid, and -- key != nullptr, grid usable -- every point's key.  Returns the number of gridded points.
inline size_t host_grid(const double* xyz, size_t n, size_t stride, double length, Grid* grid, uint64_t* key) {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    size_t n_gridded = 0;
    for (size_t i = 0; i < n; ++i) {
        const double* p = xyz + i * stride;
        if (!gridded(p[0], p[1], p[2])) continue;
        for (int c = 0; c < 3; ++c) {
            if (!n_gridded || p[c] < lo[c]) lo[c] = p[c];
            if (!n_gridded || p[c] > hi[c]) hi[c] = p[c];
        }
        ++n_gridded;
    }
    *grid = make_grid(lo, hi, n_gridded > 0, length);
    if (key)
        for (size_t i = 0; i < n; ++i) {
            const double* p = xyz + i * stride;
            key[i] = grid->usable ? body_key(*grid, p[0], p[1], p[2]) : kNoKey;
        }
    return n_gridded;
}

}}  // namespace nbody::cells

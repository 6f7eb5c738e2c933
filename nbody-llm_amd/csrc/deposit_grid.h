// deposit_grid.h -- the arithmetic of nbody_deposit and nbody_host_deposit (include/nbody_hip.h, "grid deposit"), stated once:
// the kernels (kernels_deposit.hip), the host call (nbody_deposit.cpp) and tools/sanitize_deposit.cpp all evaluate these
// functions, and tests/deposit_ref.py restates them in numpy.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off.  All of it is f64 and every operation
// is rounded on its own, so the device, the host and the restatement give the same bits:
//     u_c      (x_c - origin_c) / spacing                      per axis that is not ignored (project_axis)
//     SKIPPED  any of x, y, z, q not finite, or !(|u_c| < 2^31) on an axis that is not ignored
//     NGP      i = floor(u), weight 1
//     CIC      s = u - 0.5, i0 = floor(s), f = s - i0: cells i0, i0 + 1 with weights 1.0 - f, f
//     TSC      i = floor(u), d = (u - i) - 0.5, a = 0.5 - d, b = 0.5 + d: cells i - 1, i, i + 1 with weights
//              0.5 (a a), 0.75 - d d, 0.5 (b b)
//     the ignored axis: one cell, index 0, weight 1.0
//     term     t = q ((wx wy) wz) into cell (ix, iy, iz); periodic: every index mod dims_c into [0, dims_c); else a term whose
//              cell is off the grid is dropped
//     INSIDE   every stencil cell of the body lands on the grid (zero weights included); OUTSIDE: none does; else PARTIAL
//     scale    n = the live bodies (skipped ones included), L = ceil(log2(n)) (0 for n = 1), e = the frexp exponent of the
//              largest |q| among the bodies that are not skipped (0 when that is 0), S = 61 - e - L
//     k        llrint(ldexp(t, S)), ties to even, added to the cell's int64 by integer addition
//     grid[c]  ldexp((double) acc[c], -S)
// DESIGN 3.24 proves that no cell can overflow.
#pragma once

#include "../../include/nbody_hip.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#if defined(__HIPCC__)
#define DEPOSIT_HD __host__ __device__ inline __attribute__((always_inline))
#define DEPOSIT_UNROLL _Pragma("unroll")   // (the per-axis arrays of a Stencil stay in registers on the device)
#else
#define DEPOSIT_HD inline
#define DEPOSIT_UNROLL
#endif

namespace nbody { namespace deposit {

constexpr double kIndexLimit = 2147483648.0;   // 2^31: a body whose |u| reaches it on a used axis is skipped
constexpr int kScaleBits = 61;

// the spec as the kernels take it (by value): checked, dims[project_axis] == 1
struct Grid {
    double origin[3];
    double spacing;
    int dims[3];
    int scheme, periodic, axis;
};

DEPOSIT_HD Grid grid_of(const NbodyGridSpec& s) {
    Grid g;
    for (int c = 0; c < 3; ++c) { g.origin[c] = s.origin[c]; g.dims[c] = s.dims[c]; }
    g.spacing = s.spacing;
    g.scheme = s.scheme;
    g.periodic = s.periodic != 0;
    g.axis = s.project_axis;
    return g;
}

DEPOSIT_HD size_t cells_of(const Grid& g) { return size_t(g.dims[0]) * size_t(g.dims[1]) * size_t(g.dims[2]); }

DEPOSIT_HD bool finite64(double v) { return v - v == 0.0; }   // (false for NaN and for either infinity)

// the stencil of one body: per axis `cnt` cells from index `first` on with weights w; on[c] = how many of them land on the
// grid (all of them when periodic)
struct Stencil {
    long long first[3];
    int cnt[3];
    int on[3];
    double w[3][3];
};

enum { kInside = 0, kPartial = 1, kOutside = 2, kSkipped = 3 };

// one axis of a body's stencil (constant indices only, so that a Stencil and the Grid stay in registers on the device);
// false: the body is skipped on this axis
DEPOSIT_HD bool axis_stencil(double x, double origin, double spacing, int dim, int scheme, int periodic, bool ignored, long long* first,
                             int* cnt, int* on, double* w) {
    if (ignored) {
        *first = 0;
        *cnt = 1;
        *on = 1;
        w[0] = 1.0;
        w[1] = w[2] = 0.0;
        return true;
    }
    const double u = (x - origin) / spacing;
    if (!(std::fabs(u) < kIndexLimit)) return false;   // (a NaN or an infinite u as well)
    if (scheme == NBODY_DEPOSIT_NGP) {
        *first = (long long)std::floor(u);
        *cnt = 1;
        w[0] = 1.0;
        w[1] = w[2] = 0.0;
    } else if (scheme == NBODY_DEPOSIT_CIC) {
        const double s = u - 0.5;
        const double i0 = std::floor(s);
        const double f = s - i0;
        *first = (long long)i0;
        *cnt = 2;
        w[0] = 1.0 - f;
        w[1] = f;
        w[2] = 0.0;
    } else {
        const double i = std::floor(u);
        const double d = (u - i) - 0.5;
        const double a = 0.5 - d, b = 0.5 + d;
        *first = (long long)i - 1;
        *cnt = 3;
        w[0] = 0.5 * (a * a);
        w[1] = 0.75 - d * d;
        w[2] = 0.5 * (b * b);
    }
    int landed = 0;
    DEPOSIT_UNROLL
    for (int k = 0; k < 3; ++k) {
        const long long i = *first + k;
        landed += k < *cnt && (periodic || (i >= 0 && i < (long long)dim));
    }
    *on = landed;
    return true;
}

// false: the body is skipped
DEPOSIT_HD bool body_stencil(const Grid& g, double x, double y, double z, double q, Stencil* st) {
    if (!(finite64(x) && finite64(y) && finite64(z) && finite64(q))) return false;
    return axis_stencil(x, g.origin[0], g.spacing, g.dims[0], g.scheme, g.periodic, g.axis == 0, &st->first[0], &st->cnt[0], &st->on[0], st->w[0]) &&
           axis_stencil(y, g.origin[1], g.spacing, g.dims[1], g.scheme, g.periodic, g.axis == 1, &st->first[1], &st->cnt[1], &st->on[1], st->w[1]) &&
           axis_stencil(z, g.origin[2], g.spacing, g.dims[2], g.scheme, g.periodic, g.axis == 2, &st->first[2], &st->cnt[2], &st->on[2], st->w[2]);
}

// kInside, kPartial or kOutside of a body that is not skipped
DEPOSIT_HD int body_class(const Stencil& st) {
    if (st.on[0] == 0 || st.on[1] == 0 || st.on[2] == 0) return kOutside;
    return st.on[0] == st.cnt[0] && st.on[1] == st.cnt[1] && st.on[2] == st.cnt[2] ? kInside : kPartial;
}

// index i of an axis of `dim` cells brought onto the grid, or -1 when the term is dropped
DEPOSIT_HD long long cell_on_axis(long long i, long long dim, int periodic) {
    if (periodic) {
        i %= dim;
        return i < 0 ? i + dim : i;
    }
    return i >= 0 && i < dim ? i : -1;
}

// the index on axis c of stencil cell k, or -1 when the term is dropped
DEPOSIT_HD long long axis_cell(const Grid& g, const Stencil& st, int c, int k) { return cell_on_axis(st.first[c] + k, g.dims[c], g.periodic); }

// the body's home cell (the first stencil cell; TSC: the middle one) brought onto the grid -- wrapped when periodic, else
// clamped: the key the bodies are sorted by.  It groups bodies whose terms meet; it never shows in the result.
DEPOSIT_HD uint32_t home_cell(const Grid& g, const Stencil& st) {
    size_t cell = 0;
    DEPOSIT_UNROLL
    for (int c = 0; c < 3; ++c) {
        long long i = st.first[c] + (st.cnt[c] == 3 ? 1 : 0);
        const long long d = g.dims[c];
        if (g.periodic) {
            i %= d;
            if (i < 0) i += d;
        } else {
            i = i < 0 ? 0 : i >= d ? d - 1 : i;
        }
        cell = cell * size_t(d) + size_t(i);
    }
    return uint32_t(cell);   // (< 2^27)
}

// ceil(log2(n)) for n >= 1
DEPOSIT_HD int ceil_log2(unsigned long long n) {
    int L = 0;
    while ((1ull << L) < n) ++L;   // (n <= 2^31)
    return L;
}

// the frexp exponent of a finite v >= 0 from its bits (0 for v == 0): v = m 2^e with 0.5 <= m < 1; subnormals included
DEPOSIT_HD int frexp_exponent(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof(u));
    u &= ~(uint64_t(1) << 63);
    if (!u) return 0;
    const int biased = int(u >> 52);
    if (biased) return biased - 1022;
    int top = 51;   // a subnormal: its highest set bit b gives 2^(b - 1074) <= v, so e = b - 1073
    while (!((u >> top) & 1)) --top;
    return top - 1073;
}

// S for n live bodies whose largest |q| is qmax
DEPOSIT_HD int scale_of(unsigned long long n, double qmax) { return kScaleBits - frexp_exponent(qmax) - ceil_log2(n ? n : 1); }

DEPOSIT_HD long long fixed_of(double t, int S) { return (long long)llrint(ldexp(t, S)); }
DEPOSIT_HD double grid_value(long long acc, int S) { return ldexp(double(acc), -S); }

// the int64 sum that stands in a cell's eight bytes of the caller's grid until the cell becomes a double (host; memcpy: the
// bytes belong to an array of doubles)
inline long long load_sum(const double* cell) {
    long long a;
    std::memcpy(&a, cell, sizeof(a));
    return a;
}
inline void store_sum(double* cell, long long a) { std::memcpy(cell, &a, sizeof(a)); }

// ---- what the host needs of the whole computation: n bodies {x, y, z} and their q onto g.  acc (may be null: counts only):
// the caller's grid of cells_of(g) doubles, whose eight bytes a cell hold the int64 sums (load_sum / store_sum), zeroed here.
// counts: {inside, partial, outside, skipped}.  Returns S.
inline int host_deposit(const Grid& g, const double* xyz, const double* q, size_t n, double* acc, uint64_t counts[4]) {
    const size_t cells = cells_of(g);
    if (acc)
        for (size_t c = 0; c < cells; ++c) store_sum(acc + c, 0);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    double qmax = 0.0;
    Stencil st;
    for (size_t i = 0; i < n; ++i) {
        if (!body_stencil(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], q[i], &st)) { ++counts[kSkipped]; continue; }
        ++counts[body_class(st)];
        const double a = std::fabs(q[i]);
        if (a > qmax) qmax = a;
    }
    const int S = scale_of(n, qmax);
    if (!acc) return S;
    for (size_t i = 0; i < n; ++i) {
        if (!body_stencil(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], q[i], &st)) continue;
        for (int a = 0; a < st.cnt[0]; ++a) {
            const long long ix = axis_cell(g, st, 0, a);
            if (ix < 0) continue;
            for (int b = 0; b < st.cnt[1]; ++b) {
                const long long iy = axis_cell(g, st, 1, b);
                if (iy < 0) continue;
                for (int c = 0; c < st.cnt[2]; ++c) {
                    const long long iz = axis_cell(g, st, 2, c);
                    if (iz < 0) continue;
                    const double t = q[i] * ((st.w[0][a] * st.w[1][b]) * st.w[2][c]);
                    const size_t cell = (size_t(ix) * size_t(g.dims[1]) + size_t(iy)) * size_t(g.dims[2]) + size_t(iz);
                    // (unsigned: the proof bounds every partial sum, and wrapping would be defined anyway)
                    store_sum(acc + cell, (long long)((unsigned long long)load_sum(acc + cell) + (unsigned long long)fixed_of(t, S)));
                }
            }
        }
    }
    return S;
}

// ---- the checks of a spec and the whole of nbody_host_deposit, here so that tools/sanitize_deposit.cpp runs the very code
// why the spec is not valid (empty: it is); check_quantity: nbody_deposit's, the host call ignores the field
inline std::string spec_refusal(const NbodyGridSpec* spec, bool check_quantity) {
    if (!spec) return "spec is NULL";
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(spec->origin[c])) return "origin[" + std::to_string(c) + "] is not finite";
    if (!(std::isfinite(spec->spacing) && spec->spacing > 0.0)) return "spacing must be finite and > 0";
    unsigned long long cells = 1;
    for (int c = 0; c < 3; ++c) {
        if (spec->dims[c] < 1) return "dims[" + std::to_string(c) + "] must be >= 1";
        cells *= (unsigned long long)spec->dims[c];   // (< 2^31 each: the product is checked before it can pass 2^58)
        if (cells > (unsigned long long)NBODY_DEPOSIT_MAX_CELLS) return "the grid has more than NBODY_DEPOSIT_MAX_CELLS (2^27) cells";
    }
    if (spec->scheme != NBODY_DEPOSIT_NGP && spec->scheme != NBODY_DEPOSIT_CIC && spec->scheme != NBODY_DEPOSIT_TSC)
        return "scheme must be NBODY_DEPOSIT_NGP (0), NBODY_DEPOSIT_CIC (1) or NBODY_DEPOSIT_TSC (2)";
    if (check_quantity && (spec->quantity < NBODY_DEPOSIT_MASS || spec->quantity > NBODY_DEPOSIT_NUMBER))
        return "quantity must be one of NBODY_DEPOSIT_MASS (0) .. NBODY_DEPOSIT_NUMBER (5)";
    if (spec->project_axis < -1 || spec->project_axis > 2) return "project_axis must be -1, 0, 1 or 2";
    if (spec->project_axis >= 0 && spec->dims[spec->project_axis] != 1) return "the dimension along project_axis must be 1";
    if (spec->reserved != 0) return "reserved must be 0";
    return std::string();
}

inline int host_call(const double* xyz, const double* q, size_t n, const NbodyGridSpec& spec, double* grid, size_t cap, uint64_t* counts) {
    const Grid g = grid_of(spec);
    const size_t cells = cells_of(g);
    if (grid && cap < cells) return int(NBODY_ERR_CAPACITY);
    uint64_t counted[4];
    // the int64 sums stand in the caller's grid (eight bytes a cell, as on the device) and become doubles in place
    const int S = host_deposit(g, xyz, q, n, grid, counted);
    if (grid)
        for (size_t c = 0; c < cells; ++c) grid[c] = grid_value(load_sum(grid + c), S);
    if (counts) std::copy(counted, counted + 4, counts);
    return int(NBODY_OK);
}

// nbody_host_deposit
inline int host_entry(const double* xyz, const double* q, size_t n, const NbodyGridSpec* spec, double* grid, size_t cap, uint64_t* counts) {
    if (!spec_refusal(spec, false).empty()) return int(NBODY_ERR_INVALID);
    if ((n && (!xyz || !q)) || n > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    return host_call(xyz, q, n, *spec, grid, cap, counts);
}

}}  // namespace nbody::deposit

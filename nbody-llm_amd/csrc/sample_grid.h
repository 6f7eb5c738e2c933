// sample_grid.h -- the arithmetic of nbody_grid_sample, nbody_grid_sample_at and nbody_host_grid_sample (include/nbody_hip.h,
// "grid sample"), stated once: the kernels (kernels_sample.hip), the host call (nbody_api.cpp) and tools/sanitize_sample.cpp all
// evaluate these functions, and tests/sample_ref.py restates them in numpy.  The transpose of the deposit: the stencil of a
// point is deposit_grid.h's body_stencil(g, x, y, z, 0.0, &st) -- the skip rule, the weights, the ignored axis and
// cell_on_axis are the deposit's own code -- and the cells are read instead of added to.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off.  All of it is f64 and every operation
// is rounded on its own, so the device, the host and the restatement give the same bits:
//     VALUE, field f     s = +0.0; for a, then b, then c innermost over the stencil, a term whose cell is dropped skipped:
//                        w = (wx[a] wy[b]) wz[c];  s = s + w G_f[cell];  out[i][f] = s
//     GRADIENT, comp. k  D_k[i] = (G[i + e_k] - G[i - e_k]) / (2.0 spacing)                                           order 2
//                        D_k[i] = (8.0 (G[i + e_k] - G[i - e_k]) - (G[i + 2 e_k] - G[i - 2 e_k])) / (12.0 spacing)     order 4
//                        the denominator formed once per call; the neighbours' indices through cell_on_axis (periodic: wrapped;
//                        else a term is dropped FOR THAT COMPONENT when a cell its difference reads is off the grid);
//                        out[i][k] = the sum of w D_k[cell] in VALUE's order; along project_axis +0.0, nothing read
//     class              SKIPPED: the stencil refuses the point; OUTSIDE: no stencil cell is on the grid (both: outputs +0.0);
//                        INSIDE: every read of every component landed -- for a gradient the stencil widened by 1 or 2 cells on
//                        every axis in use --; else PARTIAL
#pragma once

#include "deposit_grid.h"

namespace nbody { namespace sample {

using deposit::Grid;
using deposit::Stencil;
using deposit::kInside;
using deposit::kOutside;
using deposit::kPartial;
using deposit::kSkipped;

// how far a difference reaches along its axis: 0 (VALUE), 1 (order 2), 2 (order 4)
DEPOSIT_HD int reach_of(int op) { return op == NBODY_SAMPLE_GRADIENT4 ? 2 : op == NBODY_SAMPLE_GRADIENT2 ? 1 : 0; }
// the doubles of a row of out
DEPOSIT_HD int width_of(int op, int fields) { return op == NBODY_SAMPLE_VALUE ? fields : 3; }
// the differences' denominator, formed once per call
DEPOSIT_HD double denominator_of(int op, double spacing) { return (op == NBODY_SAMPLE_GRADIENT4 ? 12.0 : 2.0) * spacing; }

DEPOSIT_HD double diff2(double lo1, double hi1, double den) { return (hi1 - lo1) / den; }
DEPOSIT_HD double diff4(double lo2, double lo1, double hi1, double hi2, double den) { return (8.0 * (hi1 - lo1) - (hi2 - lo2)) / den; }

DEPOSIT_HD size_t linear_cell(const Grid& g, long long ix, long long iy, long long iz) {
    return (size_t(ix) * size_t(g.dims[1]) + size_t(iy)) * size_t(g.dims[2]) + size_t(iz);   // (< dims' product <= 2^27)
}

// D_k at the cell (ix, iy, iz) of the grid (on it) from the one-field grid G; false: a cell the difference reads is off the grid
// (the term is dropped for component k).  reads: the loads made, added to.
DEPOSIT_HD bool difference_at(const Grid& g, const double* G, int k, int reach, double den, long long ix, long long iy, long long iz,
                              double* d, unsigned long long* reads) {
    long long i[3] = {ix, iy, iz};
    const long long at = i[k], dim = g.dims[k];
    double v[4] = {0.0, 0.0, 0.0, 0.0};   // G at -2, -1, +1, +2 (order 2: the middle two)
    const int offs[4] = {-2, -1, 1, 2};
    for (int j = 0; j < 4; ++j) {
        if (reach == 1 && (j == 0 || j == 3)) continue;
        const long long n = deposit::cell_on_axis(at + offs[j], dim, g.periodic);
        if (n < 0) return false;
        i[k] = n;
        v[j] = G[linear_cell(g, i[0], i[1], i[2])];
        ++*reads;
    }
    *d = reach == 1 ? diff2(v[1], v[2], den) : diff4(v[0], v[1], v[2], v[3], den);
    return true;
}

// INSIDE, PARTIAL or OUTSIDE of a point that is not skipped
DEPOSIT_HD int point_class(const Grid& g, const Stencil& st, int reach) {
    const int base = deposit::body_class(st);
    if (base != kInside || reach == 0 || g.periodic) return base;
    bool all = true;
    DEPOSIT_UNROLL
    for (int c = 0; c < 3; ++c)
        if (c != g.axis && (st.first[c] - reach < 0 || st.first[c] + (st.cnt[c] - 1) + reach >= (long long)g.dims[c])) all = false;
    return all ? kInside : kPartial;
}

// ---- one point on the host: out[width_of(op, fields)], returns its class.  grid: [fields][cells]
inline int host_point(const Grid& g, const double* grid, int fields, int op, double den, double x, double y, double z, double* out) {
    const int width = width_of(op, fields), reach = reach_of(op);
    for (int f = 0; f < width; ++f) out[f] = 0.0;
    Stencil st;
    if (!deposit::body_stencil(g, x, y, z, 0.0, &st)) return kSkipped;
    const int cls = point_class(g, st, reach);
    if (cls == kOutside) return cls;
    const size_t cells = deposit::cells_of(g);
    unsigned long long reads = 0;
    for (int a = 0; a < st.cnt[0]; ++a) {
        const long long ix = deposit::axis_cell(g, st, 0, a);
        if (ix < 0) continue;
        for (int b = 0; b < st.cnt[1]; ++b) {
            const long long iy = deposit::axis_cell(g, st, 1, b);
            if (iy < 0) continue;
            for (int c = 0; c < st.cnt[2]; ++c) {
                const long long iz = deposit::axis_cell(g, st, 2, c);
                if (iz < 0) continue;
                const double w = (st.w[0][a] * st.w[1][b]) * st.w[2][c];
                if (op == NBODY_SAMPLE_VALUE) {
                    const size_t cell = linear_cell(g, ix, iy, iz);
                    for (int f = 0; f < fields; ++f) out[f] = out[f] + w * grid[size_t(f) * cells + cell];
                    continue;
                }
                for (int k = 0; k < 3; ++k) {
                    double d;
                    if (k == g.axis || !difference_at(g, grid, k, reach, den, ix, iy, iz, &d, &reads)) continue;
                    out[k] = out[k] + w * d;
                }
            }
        }
    }
    return cls;
}

// ---- the checks of a call and the whole of nbody_host_grid_sample, here so that tools/sanitize_sample.cpp runs the very code
// why the call is not valid (empty: it is): the spec as the deposit checks it (the quantity ignored), fields, op and the grid
inline std::string call_refusal(const NbodyGridSpec* spec, const double* grid, int fields, int op) {
    const std::string why = deposit::spec_refusal(spec, false);
    if (!why.empty()) return why;
    if (fields < 1 || fields > NBODY_SAMPLE_MAX_FIELDS) return "fields must be in 1 .. NBODY_SAMPLE_MAX_FIELDS (4)";
    if (op != NBODY_SAMPLE_VALUE && op != NBODY_SAMPLE_GRADIENT2 && op != NBODY_SAMPLE_GRADIENT4)
        return "op must be NBODY_SAMPLE_VALUE (0), NBODY_SAMPLE_GRADIENT2 (1) or NBODY_SAMPLE_GRADIENT4 (2)";
    if (op != NBODY_SAMPLE_VALUE && fields != 1) return "a gradient takes one field";
    if (size_t(fields) * deposit::cells_of(deposit::grid_of(*spec)) > size_t(NBODY_DEPOSIT_MAX_CELLS))
        return "fields times the cells of the grid exceed NBODY_DEPOSIT_MAX_CELLS (2^27)";
    if (!grid) return "grid is NULL";
    return std::string();
}

inline int host_call(const double* xyz, size_t n, const NbodyGridSpec& spec, const double* grid, int fields, int op, double* out,
                     uint8_t* cls, uint64_t* counts) {
    const Grid g = deposit::grid_of(spec);
    const double den = denominator_of(op, g.spacing);
    const size_t width = size_t(width_of(op, fields));
    uint64_t counted[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        const int c = host_point(g, grid, fields, op, den, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out + i * width);
        ++counted[c];
        if (cls) cls[i] = uint8_t(c);
    }
    if (counts) std::copy(counted, counted + 4, counts);
    return int(NBODY_OK);
}

// nbody_host_grid_sample
inline int host_entry(const double* xyz, size_t n, const NbodyGridSpec* spec, const double* grid, int fields, int op, double* out,
                      uint8_t* cls, uint64_t* counts) {
    if (!call_refusal(spec, grid, fields, op).empty()) return int(NBODY_ERR_INVALID);
    if ((n && (!xyz || !out)) || n > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    return host_call(xyz, n, *spec, grid, fields, op, out, cls, counts);
}

}}  // namespace nbody::sample

// p3m_pairs.h -- the arithmetic of nbody_p3m_field, nbody_p3m_field_at, nbody_host_p3m_field and nbody_host_p3m_table
// (include/nbody_hip.h, "P3M field"), stated once: the kernels (kernels_p3m.hip), the host call below and tools/sanitize_p3m.cpp
// all evaluate these functions, and tests/p3m_ref.py restates them in numpy.  The mesh part is pm_grid.h's composition with the
// Gaussian split in the Poisson stage's D tables (poisson_grid.h, "split"); what is new here is the short-range pair sum.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off.  All of it is f64 and every operation
// is rounded on its own, so the device, the host and the restatement give the same bits:
//     table    h = (r_cut / r_split) / 4096.0;  x_k = double(k) h, k = 0 .. 4096;  e = erfc(x_k / 2.0);
//              T[k].F = e + (x_k / SQRT_PI) exp(-((x_k x_k) / 4.0));  T[k].P = e        (std::erfc, std::exp; on the host only)
//     chain    c = the smallest power of two with double(c) spacing >= r_cut, shift = log2(c); a body's chain cell on an axis is
//              cell_on_axis(floor(u), dims, periodic) >> shift with u = (x - origin) / spacing; a body the deposit skips (x, y, z
//              or m not finite, or !(|u| < 2^31)) has none.  A caller's point takes the same rule with m = 0.0.
//     walk     target i with a chain cell (cx, cy, cz): for dx = -1, 0, +1, then dy, then dz innermost, the cell ((cx + dx) mod
//              nx', (cy + dy) mod ny', (cz + dz) mod nz') and in it the bodies in ascending row; at the bodies j == i is left out
//     term     d_c = x_j,c - x_i,c;  d_c = d_c - rint(d_c / L_c) L_c, L_c = double(dims_c) spacing;  r2 = (dx dx + dy dy) + dz dz;
//              counted iff r2 < R2, R2 = r_cut r_cut; skipped when r2 == 0 and soften == 0;
//              r = sqrt(r2), t = r (4096.0 / r_cut), k = min(int(t), 4095), fr = t - double(k);
//              Fv = T[k].F + fr (T[k + 1].F - T[k].F), Pv likewise;  s2 = r2 + soften soften, inv = 1.0 / sqrt(s2),
//              inv3 = (inv inv) inv;  a_c = a_c + ((m_j inv3) Fv) d_c;  ph = ph + (m_j inv) Pv        (sums from +0.0, in walk order)
//     short    acc_short_c = g a_c;  phi_short = 0.0 - g ph;  a target without a chain cell: +0.0 four times
// DESIGN 3.30 proves that the walk meets every pair closer than r_cut.
#pragma once

#include "pm_grid.h"

namespace nbody { namespace p3m {

constexpr int kIntervals = NBODY_P3M_TABLE_INTERVALS;
constexpr double kSqrtPi = 1.7724538509055159;   // the double next to sqrt(pi)

struct alignas(16) Entry { double F, P; };   // (16: one 128-bit load on the device)

// T[0 .. 4096]
inline void table(double r_split, double r_cut, Entry* out) {
    const double h = (r_cut / r_split) / double(kIntervals);
    for (int k = 0; k <= kIntervals; ++k) {
        const double x = double(k) * h;
        const double e = std::erfc(x / 2.0);
        out[k].F = e + (x / kSqrtPi) * std::exp(-((x * x) / 4.0));
        out[k].P = e;
    }
}

// the chain grid of a checked call
struct Chain {
    int shift;
    int dims[3];
    size_t cells() const { return size_t(dims[0]) * size_t(dims[1]) * size_t(dims[2]); }
};
inline Chain chain_of(const deposit::Grid& g, double r_cut) {
    Chain ch;
    ch.shift = 0;
    while (ch.shift < 30 && double(1 << ch.shift) * g.spacing < r_cut) ++ch.shift;
    for (int c = 0; c < 3; ++c) ch.dims[c] = g.dims[c] >> ch.shift;
    return ch;
}

// what a term reads beside the two bodies, made once per call
struct Params {
    double L[3];
    double R2, scale, soften, soften2;
};
inline Params params_of(const deposit::Grid& g, double r_cut, double soften) {
    Params p;
    for (int c = 0; c < 3; ++c) p.L[c] = double(g.dims[c]) * g.spacing;
    p.R2 = r_cut * r_cut;
    p.scale = double(kIntervals) / r_cut;
    p.soften = soften;
    p.soften2 = soften * soften;
    return p;
}

// the chain cell of a body or point, linear over ch.dims; false: it has none
DEPOSIT_HD bool chain_cell(const deposit::Grid& g, const Chain& ch, double x, double y, double z, double m, uint32_t* cell) {
    if (!(deposit::finite64(x) && deposit::finite64(y) && deposit::finite64(z) && deposit::finite64(m))) return false;
    const double ux = (x - g.origin[0]) / g.spacing, uy = (y - g.origin[1]) / g.spacing, uz = (z - g.origin[2]) / g.spacing;
    if (!(std::fabs(ux) < deposit::kIndexLimit && std::fabs(uy) < deposit::kIndexLimit && std::fabs(uz) < deposit::kIndexLimit)) return false;
    const long long cx = deposit::cell_on_axis((long long)std::floor(ux), g.dims[0], 1) >> ch.shift;
    const long long cy = deposit::cell_on_axis((long long)std::floor(uy), g.dims[1], 1) >> ch.shift;
    const long long cz = deposit::cell_on_axis((long long)std::floor(uz), g.dims[2], 1) >> ch.shift;
    *cell = uint32_t((cx * ch.dims[1] + cy) * ch.dims[2] + cz);
    return true;
}

// neighbour q = 0 .. 26 of the chain cell `cell` in the walk's order (dx outermost), wrapped
DEPOSIT_HD uint32_t chain_neighbour(const Chain& ch, uint32_t cell, int q) {
    const int cz = int(cell % uint32_t(ch.dims[2])), cy = int((cell / uint32_t(ch.dims[2])) % uint32_t(ch.dims[1])),
              cx = int(cell / (uint32_t(ch.dims[2]) * uint32_t(ch.dims[1])));
    const int nx = (cx + (q / 9 - 1) + ch.dims[0]) % ch.dims[0], ny = (cy + ((q / 3) % 3 - 1) + ch.dims[1]) % ch.dims[1],
              nz = (cz + (q % 3 - 1) + ch.dims[2]) % ch.dims[2];
    return uint32_t((nx * ch.dims[1] + ny) * ch.dims[2] + nz);
}

// the sums of one target, and the two integers nbody_p3m_field_stats reports
struct Sums {
    double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
    unsigned long long looked = 0, counted = 0;
};

DEPOSIT_HD double min_image(double d, double L) { return d - std::rint(d / L) * L; }

// partner j = (xj, yj, zj, mj) as target (xi, yi, zi) sees it
DEPOSIT_HD void pair_term(const Params& p, const Entry* T, double xi, double yi, double zi, double xj, double yj, double zj, double mj, Sums& s) {
    const double dx = min_image(xj - xi, p.L[0]), dy = min_image(yj - yi, p.L[1]), dz = min_image(zj - zi, p.L[2]);
    const double r2 = (dx * dx + dy * dy) + dz * dz;
    ++s.looked;
    if (!(r2 < p.R2)) return;
    ++s.counted;
    if (r2 == 0.0 && p.soften == 0.0) return;
    const double t = std::sqrt(r2) * p.scale;
    int k = int(t);
    if (k > kIntervals - 1) k = kIntervals - 1;
    const double fr = t - double(k);
    const Entry lo = T[k], hi = T[k + 1];
    const double Fv = lo.F + fr * (hi.F - lo.F), Pv = lo.P + fr * (hi.P - lo.P);
    const double inv = 1.0 / std::sqrt(r2 + p.soften2);
    const double w = (mj * ((inv * inv) * inv)) * Fv;
    s.ax = s.ax + w * dx;
    s.ay = s.ay + w * dy;
    s.az = s.az + w * dz;
    s.ph = s.ph + (mj * inv) * Pv;
}

// what is written for a target: {acc_short x, y, z, phi_short}
DEPOSIT_HD void short_row(double g, const Sums& s, double* out4) {
    out4[0] = g * s.ax;
    out4[1] = g * s.ay;
    out4[2] = g * s.az;
    out4[3] = 0.0 - g * s.ph;
}

// ---- the host's walk: out [n][4] at the n targets P (self: they are the bodies themselves, j == i left out); pairs (may be
// null): {partners looked at, terms with r2 < R2}
inline void host_short(const deposit::Grid& g, double r_split, double r_cut, double soften, double gconst, const double* body_xyz,
                       const double* body_m, size_t n_bodies, const double* P, size_t n, bool self, double* out, uint64_t* pairs) {
    const Chain ch = chain_of(g, r_cut);
    const Params p = params_of(g, r_cut, soften);
    std::vector<Entry> T(size_t(kIntervals) + 1);
    table(r_split, r_cut, T.data());
    const size_t ncc = ch.cells();
    // the bodies of every chain cell in ascending row: a counting sort
    std::vector<uint32_t> key(n_bodies, uint32_t(ncc));
    std::vector<size_t> start(ncc + 2, 0);
    for (size_t j = 0; j < n_bodies; ++j) {
        uint32_t c;
        if (chain_cell(g, ch, body_xyz[3 * j], body_xyz[3 * j + 1], body_xyz[3 * j + 2], body_m[j], &c)) key[j] = c;
        ++start[size_t(key[j]) + 1];
    }
    for (size_t c = 0; c <= ncc; ++c) start[c + 1] += start[c];
    std::vector<size_t> order(n_bodies), fill(start.begin(), start.end() - 1);
    for (size_t j = 0; j < n_bodies; ++j) order[fill[key[j]]++] = j;
    uint64_t looked = 0, counted = 0;
    for (size_t i = 0; i < n; ++i) {
        Sums s;
        uint32_t home;
        const double xi = P[3 * i], yi = P[3 * i + 1], zi = P[3 * i + 2];
        if (chain_cell(g, ch, xi, yi, zi, self ? body_m[i] : 0.0, &home))
            for (int q = 0; q < 27; ++q) {
                const uint32_t c = chain_neighbour(ch, home, q);
                for (size_t at = start[c]; at < start[size_t(c) + 1]; ++at) {
                    const size_t j = order[at];
                    if (self && j == i) continue;
                    pair_term(p, T.data(), xi, yi, zi, body_xyz[3 * j], body_xyz[3 * j + 1], body_xyz[3 * j + 2], body_m[j], s);
                }
            }
        else { out[4 * i] = out[4 * i + 1] = out[4 * i + 2] = out[4 * i + 3] = 0.0; continue; }
        short_row(gconst, s, out + 4 * i);
        looked += s.looked;
        counted += s.counted;
    }
    if (pairs) { pairs[0] = looked; pairs[1] = counted; }
}

// ---- the checks of a call and the whole of nbody_host_p3m_field, here so that tools/sanitize_p3m.cpp runs the very code
inline std::string call_refusal(const NbodyGridSpec* spec, const NbodyP3mSpec* p3m) {
    if (!p3m) return "p3m is NULL";
    const std::string why = pm::call_refusal(spec, &p3m->pm);
    if (!why.empty()) return why;
    if (!spec->periodic) return "the grid must be periodic";
    if (spec->project_axis != -1) return "project_axis must be -1";
    if (!(std::isfinite(p3m->r_split) && p3m->r_split > 0.0)) return "r_split must be finite and > 0";
    if (!(std::isfinite(p3m->r_cut) && p3m->r_cut >= p3m->r_split && p3m->r_cut <= 8.0 * p3m->r_split))
        return "r_cut must be finite and in r_split .. 8 r_split";
    if (!(std::isfinite(p3m->soften) && p3m->soften >= 0.0)) return "soften must be finite and >= 0";
    if (p3m->terms != NBODY_P3M_BOTH && p3m->terms != NBODY_P3M_MESH_ONLY && p3m->terms != NBODY_P3M_SHORT_ONLY)
        return "terms must be NBODY_P3M_BOTH (0), NBODY_P3M_MESH_ONLY (1) or NBODY_P3M_SHORT_ONLY (2)";
    if (p3m->reserved != 0) return "reserved must be 0";
    const Chain ch = chain_of(deposit::grid_of(*spec), p3m->r_cut);
    for (int c = 0; c < 3; ++c)
        if (ch.dims[c] < 4) return "dims[" + std::to_string(c) + "] holds fewer than 4 chain cells of r_cut";
    return std::string();
}

// acc (and phi) hold the mesh part; the short part of row i is s[4 i ..]
inline void combine(int terms, size_t n, const double* s, double* acc, double* phi) {
    for (size_t i = 0; i < n; ++i) {
        for (int c = 0; c < 3; ++c) acc[3 * i + size_t(c)] = terms == NBODY_P3M_SHORT_ONLY ? s[4 * i + size_t(c)] : acc[3 * i + size_t(c)] + s[4 * i + size_t(c)];
        if (phi) phi[i] = terms == NBODY_P3M_SHORT_ONLY ? s[4 * i + 3] : phi[i] + s[4 * i + 3];
    }
}

// on a checked call.  xyz == nullptr: the points are the bodies.  pairs (may be null): host_short's
inline int host_call(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec& spec, const NbodyP3mSpec& p3m,
                     const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts, uint64_t* pairs = nullptr) {
    // the mesh part, which also makes cls and counts whatever the terms are
    const int rc = pm::host_call(body_xyz, body_m, n_bodies, spec, p3m.pm, xyz, n_points, acc, phi, cls, counts, p3m.r_split);
    if (pairs) pairs[0] = pairs[1] = 0;
    if (rc || p3m.terms == NBODY_P3M_MESH_ONLY) return rc;
    const size_t n = xyz ? n_points : n_bodies;
    std::vector<double> s(4 * n, 0.0);
    host_short(deposit::grid_of(spec), p3m.r_split, p3m.r_cut, p3m.soften, p3m.pm.poisson.g, body_xyz, body_m, n_bodies, xyz ? xyz : body_xyz, n,
               !xyz, s.data(), pairs);
    combine(p3m.terms, n, s.data(), acc, phi);
    return int(NBODY_OK);
}

// nbody_host_p3m_field
inline int host_entry(const double* body_xyz, const double* body_m, size_t n_bodies, const NbodyGridSpec* spec, const NbodyP3mSpec* p3m,
                      const double* xyz, size_t n_points, double* acc, double* phi, uint8_t* cls, uint64_t* counts) {
    if (!call_refusal(spec, p3m).empty()) return int(NBODY_ERR_INVALID);
    if ((n_bodies && (!body_xyz || !body_m)) || n_bodies > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    if (xyz && n_points > size_t(0x7fffffff)) return int(NBODY_ERR_INVALID);
    if ((xyz ? n_points : n_bodies) && !acc) return int(NBODY_ERR_INVALID);
    return host_call(body_xyz, body_m, n_bodies, *spec, *p3m, xyz, n_points, acc, phi, cls, counts);
}

// nbody_host_p3m_table
inline int host_table(double r_split, double r_cut, double* out) {
    if (!(std::isfinite(r_split) && r_split > 0.0 && std::isfinite(r_cut) && r_cut >= r_split && r_cut <= 8.0 * r_split) || !out)
        return int(NBODY_ERR_INVALID);
    std::vector<Entry> T(size_t(kIntervals) + 1);
    table(r_split, r_cut, T.data());
    for (int k = 0; k <= kIntervals; ++k) { out[2 * k] = T[size_t(k)].F; out[2 * k + 1] = T[size_t(k)].P; }
    return int(NBODY_OK);
}

}}  // namespace nbody::p3m

// poisson_grid.h -- the arithmetic of nbody_grid_poisson and nbody_host_grid_poisson (include/nbody_hip.h, "grid Poisson"),
// stated once: the kernels (kernels_poisson.hip), the host call below and tools/sanitize_poisson.cpp all evaluate these
// functions, and tests/poisson_ref.py restates them in numpy.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off.  All of it is f64 and every operation
// is rounded on its own.  Every output is a FIXED EXPRESSION TREE of the inputs -- a butterfly has two operands and no sum
// is longer -- so the device, the host and the restatement give the same bits however the work is tiled:
//     grid      the real grid becomes complex with imaginary parts +0.0; an axis of one cell is neither transformed nor padded
//     twiddles  per transform length L = 2^p, on the HOST: T[k] = (cos(a), -sin(a)), a = (TWO_PI k) / L, k < L / 2, with
//               T[0] = (1, +0) and T[L / 4] = (+0, -1) written as constants; the table is uploaded, the device evaluates no
//               sine, no cosine and no pi.  The inverse transform uses (T.re, -T.im).
//     cmul      (w, b) -> (w.re b.re - w.im b.im, w.re b.im + w.im b.re); no shortcut for any w, not even for w = 1
//     line      radix 2, decimation in time: x[rev_p(i)] <- x[i], then for s = 1 .. p, h = 2^(s - 1), every block of 2 h
//               points and j < h:  t = cmul(w, x[j + h]), w = T[j (L / (2 h))];  x[j], x[j + h] <- x[j] + t, x[j] - t
//     3-D       the lines along z, then y, then x, forward and inverse alike; the inverse is not scaled: the one
//               multiplication by 1 / points (a power of two) is made where phi is written
//     PERIODIC  tables per axis c of n cells (n = 1: K = 0, D = 1), m = i <= n / 2 ? i : i - n, made on the host:
//                 SPECTRAL  k = (TWO_PI m) / (n spacing);  K_c[i] = k k
//                 DIFF2     v = (2 sin((PI i) / n)) / spacing;  K_c[i] = v v
//                 deconvolve = d > 0:  a = (PI m) / n, s = sin(a) / a, w = s multiplied d (scheme + 1) times from the left,
//                           D_c[i] = 1 / w, D_c[0] = 1
//               c = -((FOUR_PI g) / ((spacing spacing) spacing)), once; per mode den = (K_x[i] + K_y[j]) + K_z[l],
//               f = den == 0 ? +0.0 : c / den;  d > 0: f = f ((D_x[i] D_y[j]) D_z[l]);  phi^ = (f rho^.re, f rho^.im);
//               phi[cell] = value.re (1 / points) + 0.0   (the + 0.0 here and below: a zero result is +0.0)
//               split (nbody_p3m_field, r_split > 0; internal, no public spec reaches it): S_c[i] = exp(-(K_c[i] (r_split
//               r_split))) and D_c[i] <- D_c[i] S_c[i], one product, on the host (D_c[i] = 1 without deconvolution), and the
//               f ((D_x D_y) D_z) branch is taken whatever d is
//     ISOLATED  every axis of more than one cell padded to 2 n with +0.0; on the padded grid Kr = 1 / sqrt(r2),
//               r2 = ((dx dx + dy dy) + dz dz) + soften soften, d_c = spacing m_c, m_c = i <= n_c ? i : 2 n_c - i (0 on an axis
//               of one cell); at the origin Kr = soften > 0 ? 1 / soften : +0.0.  Kr goes through the same transform, each
//               mode is cmul(Kr^, M^), and phi[cell] = (-g) (value.re (1 / points)) + 0.0 for the nx ny nz corner.
#pragma once

#include "deposit_grid.h"

#include <vector>

namespace nbody { namespace poisson {

constexpr double kPi = 3.141592653589793;       // the double next to pi; the other two are its exact multiples
constexpr double kTwoPi = 6.283185307179586;
constexpr double kFourPi = 12.566370614359172;

struct alignas(16) Cx { double re, im; };   // (16: one 128-bit load or store on the device)

DEPOSIT_HD Cx cmul(Cx w, Cx b) { return Cx{w.re * b.re - w.im * b.im, w.re * b.im + w.im * b.re}; }

// one butterfly on (a, b) with the table's entry w (inverse: its conjugate)
DEPOSIT_HD void butterfly(Cx w, bool inverse, Cx* a, Cx* b) {
    if (inverse) w.im = -w.im;
    const Cx t = cmul(w, *b);
    const Cx lo = *a;
    *a = Cx{lo.re + t.re, lo.im + t.im};
    *b = Cx{lo.re - t.re, lo.im - t.im};
}

// the p low bits of i reversed
DEPOSIT_HD unsigned reverse_bits(unsigned i, int p) {
    unsigned r = 0;
    for (int b = 0; b < p; ++b) r |= ((i >> b) & 1u) << (p - 1 - b);
    return r;
}

DEPOSIT_HD int log2_of(size_t n) {   // n = 2^p
    int p = 0;
    while ((size_t(1) << p) < n) ++p;
    return p;
}

// the periodic multiply of one mode
DEPOSIT_HD double green_factor(double c, double kx, double ky, double kz) {
    const double den = (kx + ky) + kz;
    return den == 0.0 ? 0.0 : c / den;
}
DEPOSIT_HD Cx green_mode(double c, bool deconvolve, double kx, double ky, double kz, double dx, double dy, double dz, Cx rho) {
    double f = green_factor(c, kx, ky, kz);
    if (deconvolve) f = f * ((dx * dy) * dz);
    return Cx{f * rho.re, f * rho.im};
}

// the mirrored index of padded-axis index i (n cells, padded to 2 n; an axis of one cell: 0)
DEPOSIT_HD long long mirrored(long long i, long long n) { return n == 1 ? 0 : i <= n ? i : 2 * n - i; }

// Kr at the mirrored indices (mx, my, mz)
DEPOSIT_HD double kernel_value(double spacing, double soften, long long mx, long long my, long long mz) {
    if (mx == 0 && my == 0 && mz == 0) return soften > 0.0 ? 1.0 / soften : 0.0;
    const double dx = spacing * double(mx), dy = spacing * double(my), dz = spacing * double(mz);
    const double r2 = ((dx * dx + dy * dy) + dz * dz) + soften * soften;
    return 1.0 / std::sqrt(r2);
}

// what is written to phi (+ 0.0: a zero result is +0.0, so an all-zero grid gives +0.0 everywhere)
DEPOSIT_HD double periodic_phi(double re, double inv_points) { return re * inv_points + 0.0; }
DEPOSIT_HD double isolated_phi(double g, double re, double inv_points) { return (-g) * (re * inv_points) + 0.0; }

// ---- what the host makes once per call: the shape and the tables
struct Shape {
    int n[3];        // the grid
    int len[3];      // the transform lengths: n, or 2 n on an isolated axis of more than one cell
    bool periodic;
    size_t cells() const { return size_t(n[0]) * size_t(n[1]) * size_t(n[2]); }
    size_t points() const { return size_t(len[0]) * size_t(len[1]) * size_t(len[2]); }
};

inline Shape shape_of(const NbodyGridSpec& s) {
    Shape sh;
    sh.periodic = s.periodic != 0;
    for (int c = 0; c < 3; ++c) {
        sh.n[c] = s.dims[c];
        sh.len[c] = sh.periodic || s.dims[c] == 1 ? s.dims[c] : 2 * s.dims[c];
    }
    return sh;
}

// T of one length (L >= 2): [L / 2] entries
inline void twiddles(int L, Cx* out) {
    for (int k = 0; k < L / 2; ++k) {
        const double a = (kTwoPi * double(k)) / double(L);
        out[k] = Cx{std::cos(a), -std::sin(a)};
    }
    out[0] = Cx{1.0, 0.0};
    if (L >= 4) out[L / 4] = Cx{0.0, -1.0};
}

inline long long signed_mode(int i, int n) { return i <= n / 2 ? i : i - n; }

inline void k_table(int green, int n, double spacing, double* K) {
    for (int i = 0; i < n; ++i) {
        if (n == 1) { K[i] = 0.0; continue; }
        if (green == NBODY_POISSON_SPECTRAL) {
            const double k = (kTwoPi * double(signed_mode(i, n))) / (double(n) * spacing);
            K[i] = k * k;
        } else {
            const double v = (2.0 * std::sin((kPi * double(i)) / double(n))) / spacing;
            K[i] = v * v;
        }
    }
}

inline void d_table(int deconvolve, int scheme, int n, double* D) {
    const int power = deconvolve * (scheme + 1);
    for (int i = 0; i < n; ++i) {
        if (i == 0 || n == 1) { D[i] = 1.0; continue; }
        const double a = (kPi * double(signed_mode(i, n))) / double(n);
        const double s = std::sin(a) / a;
        double w = s;
        for (int q = 1; q < power; ++q) w = w * s;
        D[i] = 1.0 / w;
    }
}

inline double green_constant(double g, double spacing) { return -((kFourPi * g) / ((spacing * spacing) * spacing)); }

struct Tables {
    std::vector<Cx> tw[3];       // the twiddles of each axis (empty: the axis is not transformed)
    std::vector<double> K[3], D[3];   // periodic: per axis (D empty without deconvolution)
    double c = 0.0;              // periodic: green_constant
    double inv_points = 1.0;
};

// r_split > 0 (p3m_pairs.h): the Gaussian split rides in D, which is then made whatever ps.deconvolve is
inline Tables tables_of(const NbodyGridSpec& s, const NbodyPoissonSpec& ps, const Shape& sh, double r_split = 0.0) {
    Tables t;
    const bool split = sh.periodic && r_split > 0.0;
    for (int c = 0; c < 3; ++c) {
        if (sh.len[c] > 1) {
            t.tw[c].resize(size_t(sh.len[c] / 2));
            twiddles(sh.len[c], t.tw[c].data());
        }
        if (!sh.periodic) continue;
        t.K[c].resize(size_t(sh.n[c]));
        k_table(ps.green, sh.n[c], s.spacing, t.K[c].data());
        if (ps.deconvolve > 0 || split) {
            t.D[c].assign(size_t(sh.n[c]), 1.0);
            if (ps.deconvolve > 0) d_table(ps.deconvolve, s.scheme, sh.n[c], t.D[c].data());
        }
        if (split) {
            const double rr = r_split * r_split;
            for (size_t i = 0; i < t.D[c].size(); ++i) t.D[c][i] = t.D[c][i] * std::exp(-(t.K[c][i] * rr));
        }
    }
    t.c = green_constant(ps.g, s.spacing);
    t.inv_points = 1.0 / double(sh.points());
    return t;
}

// ---- the host's transform: the lines of axis c of the [len0][len1][len2] array x, one after the other
inline void host_axis(Cx* x, const Shape& sh, int c, const Cx* T, bool inverse) {
    const int L = sh.len[c];
    if (L == 1) return;
    const int p = log2_of(size_t(L));
    const size_t inner = c == 2 ? 1 : c == 1 ? size_t(sh.len[2]) : size_t(sh.len[1]) * size_t(sh.len[2]);
    const size_t outer = sh.points() / (inner * size_t(L));
    std::vector<Cx> line(size_t(L), Cx{0.0, 0.0});
    for (size_t a = 0; a < outer; ++a)
        for (size_t b = 0; b < inner; ++b) {
            Cx* base = x + a * size_t(L) * inner + b;
            for (int i = 0; i < L; ++i) line[reverse_bits(unsigned(i), p)] = base[size_t(i) * inner];
            for (int s = 1; s <= p; ++s) {
                const int h = 1 << (s - 1), step = L / (2 * h);
                for (int blk = 0; blk < L; blk += 2 * h)
                    for (int j = 0; j < h; ++j) butterfly(T[j * step], inverse, &line[size_t(blk + j)], &line[size_t(blk + j + h)]);
            }
            for (int i = 0; i < L; ++i) base[size_t(i) * inner] = line[size_t(i)];
        }
}

inline void host_transform(Cx* x, const Shape& sh, const Tables& t, bool inverse) {
    for (int c = 2; c >= 0; --c) host_axis(x, sh, c, t.tw[c].data(), inverse);
}

// ---- the checks of a call and the whole of nbody_host_grid_poisson, here so that tools/sanitize_poisson.cpp runs the very code
inline bool power_of_two(long long v) { return v >= 1 && (v & (v - 1)) == 0; }

// why the call is not valid (empty: it is)
inline std::string call_refusal(const NbodyGridSpec* spec, const NbodyPoissonSpec* ps, const double* mass, const double* phi) {
    const std::string why = deposit::spec_refusal(spec, false);
    if (!why.empty()) return why;
    for (int c = 0; c < 3; ++c)
        if (!power_of_two(spec->dims[c])) return "dims[" + std::to_string(c) + "] must be a power of two";
    const Shape sh = shape_of(*spec);
    unsigned long long points = 1;
    for (int c = 0; c < 3; ++c) {
        if (sh.len[c] > NBODY_POISSON_MAX_AXIS) return "a transform length exceeds NBODY_POISSON_MAX_AXIS (4096)";
        points *= (unsigned long long)sh.len[c];
    }
    if (points > (unsigned long long)NBODY_POISSON_MAX_POINTS) return "the transform has more than NBODY_POISSON_MAX_POINTS (2^27) points";
    if (!ps) return "ps is NULL";
    if (!std::isfinite(ps->g)) return "g is not finite";
    if (!std::isfinite(ps->soften) || ps->soften < 0.0) return "soften must be finite and >= 0";
    if (sh.periodic) {
        if (ps->soften != 0.0) return "soften must be 0 on a periodic grid";
        if (ps->green != NBODY_POISSON_SPECTRAL && ps->green != NBODY_POISSON_DIFF2)
            return "green must be NBODY_POISSON_SPECTRAL (0) or NBODY_POISSON_DIFF2 (1)";
        if (ps->deconvolve < 0 || ps->deconvolve > 2) return "deconvolve must be 0, 1 or 2";
    } else {
        if (ps->green != 0) return "green must be 0 on an isolated grid";
        if (ps->deconvolve != 0) return "deconvolve must be 0 on an isolated grid";
    }
    if (ps->reserved[0] != 0 || ps->reserved[1] != 0) return "reserved must be 0";
    if (!mass) return "mass is NULL";
    if (!phi) return "phi is NULL";
    return std::string();
}

// r_split: tables_of's
inline int host_call(const NbodyGridSpec& spec, const NbodyPoissonSpec& ps, const double* mass, double* phi, double r_split = 0.0) {
    const Shape sh = shape_of(spec);
    const Tables t = tables_of(spec, ps, sh, r_split);
    const size_t points = sh.points();
    const size_t s1 = size_t(sh.len[1]) * size_t(sh.len[2]), s2 = size_t(sh.len[2]);
    std::vector<Cx> x(points, Cx{0.0, 0.0});
    for (int i = 0; i < sh.n[0]; ++i)
        for (int j = 0; j < sh.n[1]; ++j)
            for (int l = 0; l < sh.n[2]; ++l)
                x[size_t(i) * s1 + size_t(j) * s2 + size_t(l)].re = mass[(size_t(i) * size_t(sh.n[1]) + size_t(j)) * size_t(sh.n[2]) + size_t(l)];
    host_transform(x.data(), sh, t, false);
    if (sh.periodic) {
        const bool dec = ps.deconvolve > 0 || r_split > 0.0;
        for (int i = 0; i < sh.n[0]; ++i)
            for (int j = 0; j < sh.n[1]; ++j)
                for (int l = 0; l < sh.n[2]; ++l) {
                    Cx& m = x[size_t(i) * s1 + size_t(j) * s2 + size_t(l)];
                    m = green_mode(t.c, dec, t.K[0][size_t(i)], t.K[1][size_t(j)], t.K[2][size_t(l)], dec ? t.D[0][size_t(i)] : 1.0,
                                   dec ? t.D[1][size_t(j)] : 1.0, dec ? t.D[2][size_t(l)] : 1.0, m);
                }
    } else {
        std::vector<Cx> k(points, Cx{0.0, 0.0});
        for (int i = 0; i < sh.len[0]; ++i)
            for (int j = 0; j < sh.len[1]; ++j)
                for (int l = 0; l < sh.len[2]; ++l)
                    k[size_t(i) * s1 + size_t(j) * s2 + size_t(l)].re =
                        kernel_value(spec.spacing, ps.soften, mirrored(i, sh.n[0]), mirrored(j, sh.n[1]), mirrored(l, sh.n[2]));
        host_transform(k.data(), sh, t, false);
        for (size_t e = 0; e < points; ++e) x[e] = cmul(k[e], x[e]);
    }
    host_transform(x.data(), sh, t, true);
    for (int i = 0; i < sh.n[0]; ++i)
        for (int j = 0; j < sh.n[1]; ++j)
            for (int l = 0; l < sh.n[2]; ++l) {
                const double re = x[size_t(i) * s1 + size_t(j) * s2 + size_t(l)].re;
                phi[(size_t(i) * size_t(sh.n[1]) + size_t(j)) * size_t(sh.n[2]) + size_t(l)] =
                    sh.periodic ? periodic_phi(re, t.inv_points) : isolated_phi(ps.g, re, t.inv_points);
            }
    return int(NBODY_OK);
}

// nbody_host_grid_poisson
inline int host_entry(const NbodyGridSpec* spec, const NbodyPoissonSpec* ps, const double* mass, double* phi, size_t cap) {
    if (!call_refusal(spec, ps, mass, phi).empty()) return int(NBODY_ERR_INVALID);
    if (cap < shape_of(*spec).cells()) return int(NBODY_ERR_CAPACITY);
    return host_call(*spec, *ps, mass, phi);
}

// nbody_host_poisson_twiddles
inline int host_twiddles(int length, double* out) {
    if (length < 2 || length > NBODY_POISSON_MAX_AXIS || !power_of_two(length) || !out) return int(NBODY_ERR_INVALID);
    std::vector<Cx> t(size_t(length / 2));
    twiddles(length, t.data());
    for (int k = 0; k < length / 2; ++k) { out[2 * k] = t[size_t(k)].re; out[2 * k + 1] = t[size_t(k)].im; }
    return int(NBODY_OK);
}

}}  // namespace nbody::poisson

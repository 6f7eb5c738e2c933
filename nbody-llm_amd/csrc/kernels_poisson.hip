// kernels_poisson.hip -- nbody_grid_poisson on the device (gfx950): a hand-written radix-2 f64 FFT along each axis of the
// padded complex grid and the Green's-function multiply (include/nbody_hip.h, "grid Poisson").  Compiled with
// -ffp-contract=off; the arithmetic is poisson_grid.h's.  Every output point is a fixed expression tree of the input points
// and the uploaded tables, so nothing here can change a bit of the result: how many lines a block takes, where it keeps them,
// which lane does which butterfly.  No floating-point atomics; every kernel writes the call's scratch only.
//
//   k_poisson_load       x = (real, +0.0) in the nx ny nz corner of the padded grid, (+0.0, +0.0) elsewhere
//   k_poisson_kernel     k = (Kr, +0.0) on the padded grid (isolated)
//   k_poisson_fft_lds    the default plan: a block holds whole lines of one axis in LDS -- reversed on the way in, all stages out
//                        of LDS with a barrier between two stages, written back.  Lines that lie one after the other in memory
//                        (inner == 1): a block takes adjacent lines, its loads and stores are one contiguous run.  Strided
//                        lines (y and x): a block takes a tile of z-adjacent lines, point i of line t at LDS index i T + t, and
//                        lane e of a pass over the tile touches line e % T, so the global accesses are runs of 16 T bytes and
//                        every butterfly stage reads and writes T adjacent LDS points.  The LDS image is padded by one point
//                        in 16 and one in 256 (slot()): the reversed store of a line would otherwise put 16 lanes on one bank.
//   k_poisson_bitrev,    the plain plan: the reversal as swaps over global memory, then one launch per stage, one lane per
//   k_poisson_fft_stage  butterfly
//   k_poisson_green      x *= the periodic Green's function of the mode, from the per-axis tables
//   k_poisson_mul        x = cmul(k, x) (isolated)
//   k_poisson_store      real = phi of the corner: the scale, and -g when isolated
#include "kernels_poisson.h"
#include "kernels.h"   // tuning()
#include "scratch_carve.h"

#include <algorithm>

namespace nbody {

using poisson::Cx;
using poisson::kPoissonBlock;

namespace {

// where point e of a block's lines stands in its LDS image
__device__ __forceinline__ unsigned slot(unsigned e) { return e + (e >> 4) + (e >> 8); }
constexpr int slots_for(int points) { return points + points / 16 + points / 256; }

__device__ __forceinline__ unsigned reversed(unsigned i, int p) { return __brev(i) >> (32 - p); }   // (p >= 1)

// the shape of a pass as the kernels take it: lines of 2^pL points, 2^pB points between two points of a line
struct Pass {
    int pL, pB;
};

}  // namespace

__global__ __launch_bounds__(kPoissonBlock) void k_poisson_load(const double* __restrict__ real, Cx* __restrict__ x, int n0, int n1, int n2, int p1, int p2,
                                                                size_t points) {
    const size_t e = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (e >= points) return;
    const int l = int(e & ((size_t(1) << p2) - 1)), j = int((e >> p2) & ((size_t(1) << p1) - 1)), i = int(e >> (p1 + p2));
    const bool in = i < n0 && j < n1 && l < n2;
    x[e] = Cx{in ? real[(size_t(i) * size_t(n1) + size_t(j)) * size_t(n2) + size_t(l)] : 0.0, 0.0};
}

__global__ __launch_bounds__(kPoissonBlock) void k_poisson_kernel(Cx* __restrict__ k, int n0, int n1, int n2, int p1, int p2, size_t points,
                                                                  double spacing, double soften) {
    const size_t e = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (e >= points) return;
    const long long l = (long long)(e & ((size_t(1) << p2) - 1)), j = (long long)((e >> p2) & ((size_t(1) << p1) - 1)), i = (long long)(e >> (p1 + p2));
    k[e] = Cx{poisson::kernel_value(spacing, soften, poisson::mirrored(i, n0), poisson::mirrored(j, n1), poisson::mirrored(l, n2)), 0.0};
}

// One block: 2^pT lines of 2^pL points, at most kCap points in all.  !kStrided: block b takes the lines b 2^pT .. of lines that
// lie one after the other.  kStrided: the grid is [outer][2^pL][2^pB] and block b takes the 2^pT lines from inner index
// (b % tiles) 2^pT on of outer index b / tiles, tiles = 2^(pB - pT).
template <int kCap, bool kStrided>
__global__ __launch_bounds__(kPoissonBlock) void k_poisson_fft_lds(Cx* __restrict__ x, const Cx* __restrict__ T, int pL, int pB, int pT, int inverse) {
    __shared__ Cx lds[slots_for(kCap)];
    const unsigned L = 1u << pL, lines = 1u << pT, E = L << pT;   // (E <= kCap: the launcher's choice of pT and kCap)
    size_t base;
    if (kStrided) {
        const unsigned tiles_log = unsigned(pB - pT);
        const size_t outer = size_t(blockIdx.x) >> tiles_log, tile = size_t(blockIdx.x) & ((size_t(1) << tiles_log) - 1);
        base = (outer << (pL + pB)) + (tile << pT);
    } else {
        base = size_t(blockIdx.x) * E;
    }
    // in: consecutive lanes read consecutive points of memory; point i of a line goes to place rev(i)
    for (unsigned e = threadIdx.x; e < E; e += kPoissonBlock) {
        if (kStrided) {
            const unsigned i = e >> pT, t = e & (lines - 1);
            lds[slot((reversed(i, pL) << pT) + t)] = x[base + (size_t(i) << pB) + t];
        } else {
            const unsigned i = e & (L - 1), r = e >> pL;
            lds[slot((r << pL) + reversed(i, pL))] = x[base + e];
        }
    }
    __syncthreads();
    for (int s = 1; s <= pL; ++s) {
        const unsigned h = 1u << (s - 1);
        for (unsigned w = threadIdx.x; w < E / 2; w += kPoissonBlock) {
            // butterfly j of line `line`; strided: the line varies fastest over the lanes, so they touch adjacent LDS points
            const unsigned line = kStrided ? w & (lines - 1) : w >> (pL - 1);
            const unsigned j = kStrided ? w >> pT : w & (L / 2 - 1);
            const unsigned k = j & (h - 1);
            const unsigned ia = ((j >> (s - 1)) << s) + k, ib = ia + h;
            const unsigned ea = slot(kStrided ? (ia << pT) + line : (line << pL) + ia);
            const unsigned eb = slot(kStrided ? (ib << pT) + line : (line << pL) + ib);
            Cx a = lds[ea], b = lds[eb];
            poisson::butterfly(T[k << (pL - s)], inverse != 0, &a, &b);
            lds[ea] = a;
            lds[eb] = b;
        }
        __syncthreads();
    }
    for (unsigned e = threadIdx.x; e < E; e += kPoissonBlock) {
        if (kStrided) {
            const unsigned i = e >> pT, t = e & (lines - 1);
            x[base + (size_t(i) << pB) + t] = lds[slot(e)];
        } else {
            x[base + e] = lds[slot(e)];
        }
    }
}

// the reversal in place: the lane of point i < rev(i) swaps the two
__global__ __launch_bounds__(kPoissonBlock) void k_poisson_bitrev(Cx* __restrict__ x, int pL, int pB, size_t points) {
    const size_t e = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (e >= points) return;
    const unsigned i = unsigned((e >> pB) & ((size_t(1) << pL) - 1)), r = reversed(i, pL);
    if (i >= r) return;
    const size_t o = e + (size_t(r - i) << pB);   // (the same line: only the index along it differs)
    const Cx a = x[e], b = x[o];
    x[e] = b;
    x[o] = a;
}

// stage s of every line: one lane per butterfly
__global__ __launch_bounds__(kPoissonBlock) void k_poisson_fft_stage(Cx* __restrict__ x, const Cx* __restrict__ T, int pL, int pB, int s, int inverse,
                                                                     size_t butterflies) {
    const size_t w = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (w >= butterflies) return;
    const size_t inner = w & ((size_t(1) << pB) - 1), outer = w >> (pB + pL - 1);
    const unsigned j = unsigned((w >> pB) & ((size_t(1) << (pL - 1)) - 1));
    const unsigned h = 1u << (s - 1), k = j & (h - 1);
    const unsigned ia = ((j >> (s - 1)) << s) + k;
    const size_t ea = (((outer << pL) + ia) << pB) + inner, eb = ea + (size_t(h) << pB);
    Cx a = x[ea], b = x[eb];
    poisson::butterfly(T[k << (pL - s)], inverse != 0, &a, &b);
    x[ea] = a;
    x[eb] = b;
}

__global__ __launch_bounds__(kPoissonBlock) void k_poisson_green(Cx* __restrict__ x, int p1, int p2, size_t points, double c, int deconvolve,
                                                                 const double* __restrict__ K0, const double* __restrict__ K1,
                                                                 const double* __restrict__ K2, const double* __restrict__ D0,
                                                                 const double* __restrict__ D1, const double* __restrict__ D2) {
    const size_t e = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (e >= points) return;
    const size_t l = e & ((size_t(1) << p2) - 1), j = (e >> p2) & ((size_t(1) << p1) - 1), i = e >> (p1 + p2);
    const bool dec = deconvolve != 0;
    x[e] = poisson::green_mode(c, dec, K0[i], K1[j], K2[l], dec ? D0[i] : 1.0, dec ? D1[j] : 1.0, dec ? D2[l] : 1.0, x[e]);
}

__global__ __launch_bounds__(kPoissonBlock) void k_poisson_mul(Cx* __restrict__ x, const Cx* __restrict__ k, size_t points) {
    const size_t e = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (e >= points) return;
    x[e] = poisson::cmul(k[e], x[e]);
}

__global__ __launch_bounds__(kPoissonBlock) void k_poisson_store(const Cx* __restrict__ x, double* __restrict__ real, int n1, int n2, int p1, int p2,
                                                                 size_t cells, int periodic, double g, double inv_points) {
    const size_t c = size_t(blockIdx.x) * kPoissonBlock + threadIdx.x;
    if (c >= cells) return;
    const size_t l = c % size_t(n2), j = (c / size_t(n2)) % size_t(n1), i = c / (size_t(n1) * size_t(n2));
    const double re = x[(((i << p1) + j) << p2) + l].re;
    real[c] = periodic ? poisson::periodic_phi(re, inv_points) : poisson::isolated_phi(g, re, inv_points);
}

namespace poisson {

namespace {

dim3 blocks_for(size_t n) { return dim3(unsigned((n + kPoissonBlock - 1) / kPoissonBlock)); }

size_t floor_pow2(size_t v) {
    size_t p = 1;
    while (2 * p <= v) p *= 2;
    return p;
}

Scratch layout(Carver& c, const Shape& sh, bool deconvolve, bool own_real) {
    Scratch w;
    if (own_real) w.real = c.take<double>(sh.cells());
    w.x = c.take<Cx>(sh.points());
    if (!sh.periodic) w.k = c.take<Cx>(sh.points());
    for (int a = 0; a < 3; ++a) {
        if (sh.len[a] > 1) w.tw[a] = c.take<Cx>(size_t(sh.len[a] / 2));
        if (!sh.periodic) continue;
        w.K[a] = c.take<double>(size_t(sh.n[a]));
        if (deconvolve) w.D[a] = c.take<double>(size_t(sh.n[a]));
    }
    return w;
}

}  // namespace

Plan make_plan() {
    const Tuning& t = nbody::tuning();
    Plan p;
    p.lds = t.poisson_lds != 0;
    p.tile = int(floor_pow2(size_t(std::min(std::max(t.poisson_tile, 1), kMaxTile))));
    return p;
}

int lines_per_block(const Plan& p, size_t L, size_t inner, size_t lines) {
    if (inner == 1) return int(std::min(lines, std::max<size_t>(1, size_t(kLdsPointsSmall) / L)));
    return int(std::min({size_t(p.tile), inner, size_t(kLdsPoints) / L}));   // (all three powers of two, L <= kLdsPoints)
}

size_t scratch_bytes(const Shape& sh, bool deconvolve, bool own_real) { Carver c; layout(c, sh, deconvolve, own_real); return c.offset(); }
Scratch scratch_layout(void* base, const Shape& sh, bool deconvolve, bool own_real) {
    Carver c(base);
    return layout(c, sh, deconvolve, own_real);
}

void launch_load(hipStream_t s, const Shape& sh, const Scratch& w) {
    const size_t points = sh.points();
    hipLaunchKernelGGL(k_poisson_load, blocks_for(points), dim3(kPoissonBlock), 0, s, w.real, w.x, sh.n[0], sh.n[1], sh.n[2], log2_of(size_t(sh.len[1])),
                       log2_of(size_t(sh.len[2])), points);
}

void launch_kernel(hipStream_t s, const Shape& sh, double spacing, double soften, const Scratch& w) {
    const size_t points = sh.points();
    hipLaunchKernelGGL(k_poisson_kernel, blocks_for(points), dim3(kPoissonBlock), 0, s, w.k, sh.n[0], sh.n[1], sh.n[2], log2_of(size_t(sh.len[1])),
                       log2_of(size_t(sh.len[2])), points, spacing, soften);
}

int launch_transform(hipStream_t s, const Shape& sh, const Plan& p, Cx* x, const Scratch& w, bool inverse) {
    const size_t points = sh.points();
    int launches = 0;
    for (int c = 2; c >= 0; --c) {
        const size_t L = size_t(sh.len[c]);
        if (L == 1) continue;
        const size_t inner = c == 2 ? 1 : c == 1 ? size_t(sh.len[2]) : size_t(sh.len[1]) * size_t(sh.len[2]);
        const int pL = log2_of(L), pB = log2_of(inner), inv = inverse ? 1 : 0;
        if (!p.lds) {
            hipLaunchKernelGGL(k_poisson_bitrev, blocks_for(points), dim3(kPoissonBlock), 0, s, x, pL, pB, points);
            for (int st = 1; st <= pL; ++st, ++launches)
                hipLaunchKernelGGL(k_poisson_fft_stage, blocks_for(points / 2), dim3(kPoissonBlock), 0, s, x, w.tw[c], pL, pB, st, inv, points / 2);
            continue;
        }
        const size_t per = size_t(lines_per_block(p, L, inner, points / L));
        const int pT = log2_of(per);
        const bool small = per * L <= size_t(kLdsPointsSmall);
        const dim3 grid(unsigned(points / (per * L))), block(kPoissonBlock);
        if (inner == 1) {
            if (small) hipLaunchKernelGGL((k_poisson_fft_lds<kLdsPointsSmall, false>), grid, block, 0, s, x, w.tw[c], pL, pB, pT, inv);
            else hipLaunchKernelGGL((k_poisson_fft_lds<kLdsPoints, false>), grid, block, 0, s, x, w.tw[c], pL, pB, pT, inv);
        } else {
            if (small) hipLaunchKernelGGL((k_poisson_fft_lds<kLdsPointsSmall, true>), grid, block, 0, s, x, w.tw[c], pL, pB, pT, inv);
            else hipLaunchKernelGGL((k_poisson_fft_lds<kLdsPoints, true>), grid, block, 0, s, x, w.tw[c], pL, pB, pT, inv);
        }
        ++launches;
    }
    return launches;
}

void launch_green(hipStream_t s, const Shape& sh, double c, bool deconvolve, const Scratch& w) {
    const size_t points = sh.points();
    hipLaunchKernelGGL(k_poisson_green, blocks_for(points), dim3(kPoissonBlock), 0, s, w.x, log2_of(size_t(sh.len[1])), log2_of(size_t(sh.len[2])), points, c,
                       deconvolve ? 1 : 0, w.K[0], w.K[1], w.K[2], w.D[0], w.D[1], w.D[2]);
}

void launch_mul(hipStream_t s, const Shape& sh, const Scratch& w) {
    const size_t points = sh.points();
    hipLaunchKernelGGL(k_poisson_mul, blocks_for(points), dim3(kPoissonBlock), 0, s, w.x, w.k, points);
}

void launch_store(hipStream_t s, const Shape& sh, double g, double inv_points, const Scratch& w) {
    const size_t cells = sh.cells();
    hipLaunchKernelGGL(k_poisson_store, blocks_for(cells), dim3(kPoissonBlock), 0, s, w.x, w.real, sh.n[1], sh.n[2], log2_of(size_t(sh.len[1])),
                       log2_of(size_t(sh.len[2])), cells, sh.periodic ? 1 : 0, g, inv_points);
}

}}  // namespace nbody::poisson

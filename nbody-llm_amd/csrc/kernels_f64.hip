// kernels_f64.hip -- the tree walks and the energy diagnostic of the path with F = f64 (the reference's trait is generic
// over Float, shared.rs:12-44, and its own driver instantiates f64: src/main.rs:52-105).  The strict walks keep the
// reference's rounding sequence in double precision, bit for bit against the oracle's f64 instantiation and the committed
// *_f64_* golden vectors; they are kernels_bh.hip's shapes (k_bh_walk_nested / k_bh_walk<false, DIRECT>) with double4 state
// and 64-byte node records.  K0, K1, K3 and K4 of an f64 handle are the templated kernels of kernels_integrate.hip (the
// look-back retain: retain.h), K2 strict is kernels_bf.hip's k_bf_strict<double>; their f64 launchers sit next to them.
// Compiled with -ffp-contract=off; f64 sqrt and divide are correctly rounded on gfx950.
#include "kernels_f64.h"
#include "kernels.h"   // nbody::tuning()
#include "kernels_field.h"
#include "probe_term.h"
#include "walk_common.h"

#include <algorithm>

namespace nbody64 {

namespace {

using nbody::add_walk_counts;
using nbody::nearest_first_segment;

// ---- K5: BarnesHutSimulation::calc_force (barnes_hut.rs:185-203) with the reference's nested sums (see
// kernels_bh.hip k_bh_walk_nested): the innermost open cell's sum in registers, the outer ones on a per-lane stack
constexpr int kWalkBlock = 64;

__global__ __launch_bounds__(kWalkBlock) void k_bh_walk_nested(const Node64* __restrict__ nodes, const int* __restrict__ order, int n_order,
                                                               const double4* __restrict__ pos, double4* __restrict__ acc, double g,
                                                               double eps2, double theta2, unsigned long long* __restrict__ counters,
                                                               Open64* __restrict__ stack, size_t stack_stride) {
    const int t = blockIdx.x * kWalkBlock + threadIdx.x;
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n_order) {
        const int b = order[t];
        const double4 p = pos[b];
        double sx = 0.0, sy = 0.0, sz = 0.0;   // the innermost open cell's running sum
        int end = 0;                           // ... and the index after its subtree
        int d = 0;                             // open cells
        double ox = 0.0, oy = 0.0, oz = 0.0;   // calc_force(root)
        int i = 0;
        bool done = false;
        while (!done) {
            const Node64 nd = nodes[i];
            const double rx = nd.x - p.x, ry = nd.y - p.y, rz = nd.z - p.z;    // :190
            const double r2 = (rx * rx + ry * ry) + rz * rz;                     // :191
            const int skip = nd.skip;
            ++n_vis;
            double fx = 0.0, fy = 0.0, fz = 0.0;
            bool value = true;               // this visit yields a value for the enclosing cell
            if (nd.w2 < theta2 * r2) {                                           // :192
                const double r_dist = __builtin_sqrt(r2 + eps2);                 // :193
                const double r_cubed = r_dist * r_dist * r_dist;                 // :194
                const double k = ((g * nd.m) / r_cubed);                         // :195
                fx = rx * k; fy = ry * k; fz = rz * k;
                ++n_acc;
                i = skip;
            } else if (skip == i + 1) {      // a leaf (or the empty root): the fold of nothing is 0 (:197-202)
                i = skip;
            } else {                         // open the cell: its children fold into a fresh sum
                if (d > 0) stack[size_t(d) * stack_stride + t] = Open64{sx, sy, sz, end, 0};
                ++d;
                sx = sy = sz = 0.0;
                end = skip;
                i = i + 1;
                value = false;
            }
            if (value) {
                if (d == 0) { ox = fx; oy = fy; oz = fz; done = true; }        // the root itself was accepted (or is a leaf)
                else { sx += fx; sy += fy; sz += fz; }                          // acc += child result
            }
            while (!done && d > 0 && i == end) {   // the innermost cell is finished: hand its sum up
                const double vx = sx, vy = sy, vz = sz;
                --d;
                if (d == 0) { ox = vx; oy = vy; oz = vz; done = true; }
                else {
                    const Open64 up = stack[size_t(d) * stack_stride + t];
                    sx = up.x + vx; sy = up.y + vy; sz = up.z + vz;
                    end = up.end;
                }
            }
        }
        acc[b] = make_double4(ox, oy, oz, 0.0);  // :260
    }
    add_walk_counts(counters, blockIdx.x, n_acc, n_vis);
}

// NBODY_LEAF_DIRECT: the walk of src/llm/barnes_hut.rs:915-997 on the same tree, one running sum in visit order
__global__ __launch_bounds__(kWalkBlock) void k_bh_walk_direct(const Node64* __restrict__ nodes, int n_nodes, const int* __restrict__ order,
                                                               int n_order, const double4* __restrict__ pos, double4* __restrict__ acc,
                                                               double g, double eps2, double theta2,
                                                               unsigned long long* __restrict__ counters) {
    const int t = blockIdx.x * kWalkBlock + threadIdx.x;
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n_order) {
        const int b = order[t];
        const double4 p = pos[b];
        double ax = 0.0, ay = 0.0, az = 0.0;
        int i = 0;
        while (i < n_nodes) {
            const Node64 nd = nodes[i];
            const double rx = nd.x - p.x, ry = nd.y - p.y, rz = nd.z - p.z;
            const double r2 = (rx * rx + ry * ry) + rz * rz;
            ++n_vis;
            const int skip = nd.skip;
            if (r2 < 1e-10) { i = skip; continue; }                              // llm :933-935 (the body's own leaf: r2 = 0)
            if (nd.w2 < theta2 * r2 || skip == i + 1) {                          // llm :938 accepted cell, :958-972 leaf
                const double inv_r = 1.0 / __builtin_sqrt(r2 + eps2);            // llm :942
                const double inv_r3 = inv_r * inv_r * inv_r;                     // llm :944
                const double k = g * nd.m * inv_r3;                              // llm :947
                ax += rx * k; ay += ry * k; az += rz * k;                        // llm :950-952
                ++n_acc;
                i = skip;
            } else {
                i = i + 1;
            }
        }
        acc[b] = make_double4(ax, ay, az, 0.0);
    }
    add_walk_counts(counters, blockIdx.x, n_acc, n_vis);
}

// ---- K5, fast arithmetic: the opening tests are the reference's (same products, same comparison: node counts stay
// exact on the host-built tree), the accepted monopoles are added into one running sum per lane with FMAs and 1/sqrt
__device__ __forceinline__ int walk_entry64(const Node64* __restrict__ nodes, const WalkSplit64& sp, int seg, const double4 p, double theta2, bool direct) {
    const int na = sp.n_anc[seg];
    for (int k = 0; k < na; ++k) {
        const Node64 nd = nodes[sp.anc[seg * nbody::kMaxAnc + k]];
        const double rx = nd.x - p.x, ry = nd.y - p.y, rz = nd.z - p.z;
        const double r2 = (rx * rx + ry * ry) + rz * rz;
        if (direct && r2 < 1e-10) return nd.skip;
        if (nd.w2 < theta2 * r2) return nd.skip;   // accepted: the walk resumes after its subtree
    }
    return sp.first[seg];
}

// BPL neighbouring bodies of the tree order per lane, walked in lockstep: the lane visits the smallest of their next
// indices, fetches that 64-byte record once and evaluates it for whichever bodies are due there (kernels_bh.hip
// k_bh_walk_duo: per body the same tests in the same order, the same sums; per lane the union of the sequences)
template <bool DIRECT, int BPL>
__global__ __launch_bounds__(kWalkBlock) void k_bh_walk_fast64(const Node64* __restrict__ nodes, int n_nodes, const int* __restrict__ order, int n_order,
                                                               const double4* __restrict__ pos, double4* __restrict__ acc, double g, double eps2,
                                                               double theta2, unsigned long long* __restrict__ counters, WalkSplit64 split, int xcd_blocks) {
    // (xcd_blocks != 0: XCD j -- workgroups j, j + 8, ... -- walks the j-th eighth of the tree order: kernels_bh.hip k_bh_walk_duo)
    const int bx = xcd_blocks ? int(blockIdx.x % 8) * xcd_blocks + int(blockIdx.x / 8) : int(blockIdx.x);
    const int t = bx * kWalkBlock + threadIdx.x;
    // a body group's long walks are in the segments around its own place in the tree: those first (kernels_bh.hip k_bh_walk)
    const int seg = nearest_first_segment(bx, gridDim.x, blockIdx.y, gridDim.y);
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    const int t0 = BPL * t;
    if (t0 < n_order) {
        double4 p[BPL];
        double ax[BPL], ay[BPL], az[BPL];
        int nx[BPL], body[BPL];
        int i = s1;
#pragma unroll
        for (int q = 0; q < BPL; ++q) {
            const bool live = t0 + q < n_order;
            body[q] = order[live ? t0 + q : t0];
            p[q] = pos[body[q]];
            ax[q] = ay[q] = az[q] = 0.0;
            nx[q] = live ? walk_entry64(nodes, split, seg, p[q], theta2, DIRECT) : s1;
            i = min(i, nx[q]);
        }
        while (i < s1) {
            const Node64 nd = nodes[i];
            const int skip = nd.skip;
            int nxt = s1;
#pragma unroll
            for (int q = 0; q < BPL; ++q) {
                if (nx[q] == i) {
                    const double rx = nd.x - p[q].x, ry = nd.y - p[q].y, rz = nd.z - p[q].z;
                    const double r2 = (rx * rx + ry * ry) + rz * rz;
                    ++n_vis;
                    if (DIRECT && r2 < 1e-10) nx[q] = skip;
                    else if (nd.w2 < theta2 * r2 || (DIRECT && skip == i + 1)) {
                        const double rinv = rsqrt(r2 + eps2);
                        const double k = (g * nd.m) * ((rinv * rinv) * rinv);
                        ax[q] = fma(rx, k, ax[q]); ay[q] = fma(ry, k, ay[q]); az[q] = fma(rz, k, az[q]);
                        ++n_acc;
                        nx[q] = skip;
                    } else {
                        nx[q] = i + 1;
                    }
                }
                nxt = min(nxt, nx[q]);
            }
            i = nxt;
        }
#pragma unroll
        for (int q = 0; q < BPL; ++q)
            if (t0 + q < n_order)
                *(split.n_seg > 1 ? split.planes + size_t(seg) * split.plane_stride + (t0 + q) : acc + body[q]) = make_double4(ax[q], ay[q], az[q], 0.0);
    }
    add_walk_counts(counters, blockIdx.x, n_acc, n_vis);
}

// KICK: integrate_after_force (shared.rs:141-148) rides along (k_kick_drift's arithmetic, one launch less per step)
template <bool KICK>
__global__ __launch_bounds__(256) void k_bh_reduce64(const double4* __restrict__ planes, int n_seg, size_t plane_stride, const int* __restrict__ order,
                                                     int n_order, double4* __restrict__ acc, double4* __restrict__ pos, double4* __restrict__ vel, double dt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_order) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = 0; k < n_seg; ++k) {   // segment order = the order the single walk adds them in
        const double4 v = planes[size_t(k) * plane_stride + t];
        sx += v.x; sy += v.y; sz += v.z;
    }
    const int b = order[t];
    acc[b] = make_double4(sx, sy, sz, 0.0);
    if (KICK) nbody::kick_half_drift(pos, vel, b, sx, sy, sz, dt);
}

// ---- nbody_potentials(NBODY_POTENTIAL_TREE) on an f64 handle: kernels_bh.hip k_bh_pot_walk for 64-byte records -- the DIRECT
// walk's opening tests, a term m / sqrt(r2 + eps2) with IEEE sqrt and divide, one f64 entry per (segment, body)
__global__ __launch_bounds__(kWalkBlock) void k_bh_pot_walk64(const Node64* __restrict__ nodes, const int* __restrict__ order, int n_order,
                                                              const double4* __restrict__ pos, double eps2, double theta2,
                                                              unsigned long long* __restrict__ counters, WalkSplit64 split,
                                                              double* __restrict__ planes, size_t plane_stride) {
    const int t = blockIdx.x * kWalkBlock + threadIdx.x;
    const int seg = nearest_first_segment(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n_order) {
        const double4 p = pos[order[t]];
        double sum = 0.0;
        int i = walk_entry64(nodes, split, seg, p, theta2, true);
        while (i < s1) {
            const Node64 nd = nodes[i];
            const double rx = nd.x - p.x, ry = nd.y - p.y, rz = nd.z - p.z;
            const double r2 = (rx * rx + ry * ry) + rz * rz;
            const int skip = nd.skip;
            ++n_vis;
            if (r2 < 1e-10) { i = skip; continue; }
            if (nd.w2 < theta2 * r2 || skip == i + 1) {
                sum += nd.m / __builtin_sqrt(r2 + eps2);
                ++n_acc;
                i = skip;
            } else {
                i = i + 1;
            }
        }
        planes[size_t(seg) * plane_stride + t] = sum;
    }
    add_walk_counts(counters, blockIdx.x + blockIdx.y * gridDim.x, n_acc, n_vis);
}

// ---- nbody_field_at / nbody_tidal_at (NBODY_POTENTIAL_TREE) on an f64 handle: kernels_bh.hip k_bh_probe_walk for 64-byte
// records (the same tests, Term and NaN rule, all in f64)
template <class Term>
__global__ __launch_bounds__(kWalkBlock) void k_bh_probe_walk64(const Node64* __restrict__ nodes, const double* __restrict__ xyz,
                                                                const int* __restrict__ idx, int n, double eps2, double theta2,
                                                                unsigned long long* __restrict__ counters, WalkSplit64 split,
                                                                double* __restrict__ planes, size_t plane_stride) {
    const int t = blockIdx.x * kWalkBlock + threadIdx.x;
    const int seg = nearest_first_segment(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n) {
        const size_t c = size_t(idx[t]);
        const double4 p = make_double4(xyz[3 * c], xyz[3 * c + 1], xyz[3 * c + 2], 0.0);
        const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
        double sums[Term::kSums] = {};
        int i = walk_entry64(nodes, split, seg, p, theta2, true);
        while (i < s1) {
            const Node64 nd = nodes[i];
            const double rx = nd.x - p.x, ry = nd.y - p.y, rz = nd.z - p.z;
            const double r2 = (rx * rx + ry * ry) + rz * rz;
            const int skip = nd.skip;
            ++n_vis;
            if (r2 < 1e-10) { i = skip; continue; }
            if (nd.w2 < theta2 * r2 || skip == i + 1) {
                if (Term::kAny) Term::add(sums, rx, ry, rz, nd.m, r2 + eps2, false);
                ++n_acc;
                i = skip;
            } else {
                i = i + 1;
            }
        }
        if (Term::kAny) nbody::store_probe_row(planes, seg, plane_stride, t, sums, finite);
    }
    add_walk_counts(counters, blockIdx.x + blockIdx.y * gridDim.x, n_acc, n_vis);
}

// ---- diagnostics: KE and pair-potential row sums, per-block partials {KE, sum_j m_i m_j / d_ij}
constexpr int kEnergyBlock = 256;
__global__ __launch_bounds__(kEnergyBlock) void k_energy(const double4* __restrict__ pos, const double4* __restrict__ vel,
                                                         const int* __restrict__ count, double eps2, double* __restrict__ out2) {
    __shared__ double4 tile[kEnergyBlock];
    __shared__ double red[2][kEnergyBlock];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kEnergyBlock + tid;
    const int n = *count;
    const double4 pi = (i < n) ? pos[i] : make_double4(0.0, 0.0, 0.0, 0.0);
    double ke = 0.0, pe = 0.0;
    if (i < n) { const double4 v = vel[i]; ke = 0.5 * pi.w * ((v.x * v.x + v.y * v.y) + v.z * v.z); }
    for (int t0 = 0; t0 < n; t0 += kEnergyBlock) {
        __syncthreads();
        tile[tid] = (t0 + tid < n) ? pos[t0 + tid] : make_double4(0.0, 0.0, 0.0, 0.0);
        __syncthreads();
        const int cnt = min(kEnergyBlock, n - t0);
        if (i < n)
            for (int j = 0; j < cnt; ++j) {
                if (t0 + j == i) continue;
                const double4 pj = tile[j];
                const double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                pe += pi.w * pj.w / sqrt(dx * dx + dy * dy + dz * dz + eps2);
            }
    }
    red[0][tid] = ke; red[1][tid] = pe;
    __syncthreads();
    for (int off = kEnergyBlock / 2; off > 0; off >>= 1) {
        if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
        __syncthreads();
    }
    if (tid == 0) { out2[2 * blockIdx.x] = red[0][0]; out2[2 * blockIdx.x + 1] = red[1][0]; }
}

inline int blocks_for(int n, int bs) { return n <= 0 ? 0 : (n + bs - 1) / bs; }

}  // namespace

void launch_bh_walk(hipStream_t s, const Dev& d, const Node64* nodes, int n_nodes, const int* order, int n_order, double g, double eps2,
                    double theta2, unsigned long long* counters, int leaf_direct, Open64* stack, size_t stack_stride) {
    if (n_order <= 0) return;
    const dim3 grid(blocks_for(n_order, kWalkBlock));
    if (leaf_direct)
        hipLaunchKernelGGL(k_bh_walk_direct, grid, dim3(kWalkBlock), 0, s, nodes, n_nodes, order, n_order, d.own_pos(), d.acc, g, eps2, theta2, counters);
    else
        hipLaunchKernelGGL(k_bh_walk_nested, grid, dim3(kWalkBlock), 0, s, nodes, order, n_order, d.own_pos(), d.acc, g, eps2, theta2, counters,
                           stack, stack_stride);
}
void launch_bh_walk_fast(hipStream_t s, const Dev& d, const Node64* nodes, int n_nodes, const int* order, int n_order, double g, double eps2,
                         double theta2, unsigned long long* counters, int leaf_direct, const WalkSplit64& split, int bodies_per_lane, const double* kick_dt, int* kicked) {
    if (kicked) *kicked = 0;
    if (n_order <= 0) return;
    const int bpl = bodies_per_lane >= 6 ? 6 : bodies_per_lane >= 4 ? 4 : bodies_per_lane == 3 ? 3 : bodies_per_lane == 2 ? 2 : 1;
    const int gx = int(blocks_for((n_order + bpl - 1) / bpl, kWalkBlock)), gx8 = (gx + 7) / 8 * 8;
    const int xcd_blocks = nbody::tuning().bh_walk_xcd ? gx8 / 8 : 0;
    const dim3 grid(xcd_blocks ? gx8 : gx, split.n_seg);
#define WALK64(D, B) hipLaunchKernelGGL((k_bh_walk_fast64<D, B>), grid, dim3(kWalkBlock), 0, s, nodes, n_nodes, order, n_order, d.own_pos(), d.acc, g, eps2, theta2, counters, split, xcd_blocks)
#define WALK64_B(D) do { if (bpl == 6) WALK64(D, 6); else if (bpl == 4) WALK64(D, 4); else if (bpl == 3) WALK64(D, 3); else if (bpl == 2) WALK64(D, 2); else WALK64(D, 1); } while (0)
    if (leaf_direct) WALK64_B(true); else WALK64_B(false);
#undef WALK64_B
#undef WALK64
    if (split.n_seg > 1) {
        if (kick_dt) {   // (every own body is in `order` exactly once: the kick reaches them all)
            hipLaunchKernelGGL(k_bh_reduce64<true>, dim3(blocks_for(n_order, 256)), dim3(256), 0, s, split.planes, split.n_seg, split.plane_stride, order, n_order,
                               d.acc, d.own_pos(), d.vel, *kick_dt);
            if (kicked) *kicked = 1;
        } else {
            hipLaunchKernelGGL(k_bh_reduce64<false>, dim3(blocks_for(n_order, 256)), dim3(256), 0, s, split.planes, split.n_seg, split.plane_stride, order, n_order,
                               d.acc, d.own_pos(), d.vel, 0.0);
        }
    }
}
void launch_bh_pot_walk(hipStream_t s, const double4* pos, const Node64* nodes, const int* order, int n_order, double eps2, double theta2,
                        const WalkSplit64& split, double* planes, size_t plane_stride, unsigned long long* counters) {
    if (n_order <= 0) return;
    hipLaunchKernelGGL(k_bh_pot_walk64, dim3(blocks_for(n_order, kWalkBlock), split.n_seg), dim3(kWalkBlock), 0, s, nodes, order, n_order, pos,
                       eps2, theta2, counters, split, planes, plane_stride);
}
void launch_bh_probe_walk(hipStream_t s, nbody::ProbeTerm term, const nbody::FieldTree& t, const double* xyz, const int* idx, int n, double eps2,
                          double theta2, double* planes, size_t stride, unsigned long long* counters) {
    if (n <= 0) return;
    const WalkSplit64 sp{t.K, t.first, t.anc, t.n_anc, nullptr, 0};
    const dim3 grid(blocks_for(n, kWalkBlock), t.K);
    const Node64* nodes = static_cast<const Node64*>(t.nodes);
    NBODY_PROBE_TERM(term, hipLaunchKernelGGL(k_bh_probe_walk64<Term>, grid, dim3(kWalkBlock), 0, s, nodes, xyz, idx, n, eps2, theta2, counters, sp, planes, stride));
}
void launch_energy(hipStream_t s, const Dev& d, int n_upper, double eps2, double* out2) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_energy, dim3(blocks_for(n_upper, kEnergyBlock)), dim3(kEnergyBlock), 0, s, d.own_pos(), d.vel, d.own_count(), eps2, out2);
}

}  // namespace nbody64

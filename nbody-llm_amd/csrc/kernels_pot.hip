// kernels_pot.hip -- nbody_potentials(NBODY_POTENTIAL_PAIRS) and the partials of nbody_energy_world: the exact pair sum
// S_i = sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps2) for handles of either dtype.  Coordinates are widened to f64 as they
// are loaded (exact), so differences, terms and sums are f64 on f32 handles too; a term is an IEEE sqrt and an IEEE divide.
//
// The scheme is kernels_bf64.hip's with one accumulator per body instead of three:
//   k_pot_sym     a wave keeps a RESIDENT SET of 64*IPT bodies in registers; TRAVELLING CHUNKS of 64 bodies sit in the
//                 wave's LDS tile, lane l reads the one it meets and holds that body's running sum, which moves one lane
//                 per step (2 ds_bpermute_b32).  Set a meets the chunks of sets a+1 .. a+ceil(A/2)-1 (cyclic): every
//                 unordered pair between different sets at those distances is evaluated once and credited to both bodies.
//   k_pot_os      one-sided, one body per lane, partners through the wave's LDS tile (partner_stream.h).  MODE 0: every own
//                 body (small blocks); MODE 1: what k_pot_sym leaves over (the own set and, for even A, the opposite
//                 set); MODE 2: the other index blocks' bodies (between shards the sum is one-sided: the travelling side
//                 would have to be sent back to its owner, and this is a diagnostic, not the step).
//   k_pot_pairs_reduce   the planes added in plane order.
// Every plane entry is written exactly once per call and there are no atomics: the same bits from run to run.
#include "kernels_pot.h"
#include "pair64.h"
#include "partner_stream.h"

namespace nbody {

namespace {

// pad_body: where two padding bodies meet with eps2 = 0 the term is 0 * inf = NaN: it lands in the padding bodies' own rows
// (>= the live count) only, which k_pot_pairs_reduce never reads
using nbody64::pair64::pad_body;
using nbody64::pair64::rot64;

__device__ __forceinline__ double inv_dist(const double4 a, double bx, double by, double bz, double eps2) {
    const double dx = a.x - bx, dy = a.y - by, dz = a.z - bz;
    return 1.0 / __builtin_sqrt(((dx * dx + dy * dy) + dz * dz) + eps2);
}

// 4 waves per workgroup; wave gw = a * K + part is slice `part` of resident set a (kernels_bf64.hip k_bf64_sym, ROT = 0)
template <class P, int IPT>
__global__ __launch_bounds__(256) void k_pot_sym(const P* __restrict__ pos, const int* __restrict__ count, int A, int K, int sym_sets,
                                                 double* __restrict__ planes, size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= A * K) return;
    const int a = gw / K, part = gw - a * K;
    const int n = *count;
    const int Cn = A * IPT;                       // chunks in the padded body array
    const int L = IPT * sym_sets;                 // chunk visits of a set
    const int k0 = int((long long)L * part / K), k1 = int((long long)L * (part + 1) / K);
    const int src1 = ((lane + 63) & 63) * 4;      // take from the lane below
    double xi[IPT], yi[IPT], zi[IPT], mi[IPT], si[IPT];
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const int i = (a * IPT + q) * 64 + lane;
        const double4 p = (i < n) ? widen(pos[i]) : pad_body();
        xi[q] = p.x; yi[q] = p.y; zi[q] = p.z; mi[q] = p.w;
        si[q] = 0.0;
    }
    auto chunk_of = [&](int k) {
        int c = (a + 1) * IPT + k;
        if (c >= Cn) c -= Cn;
        return c;
    };
    auto load_chunk = [&](int k) {
        const int j = chunk_of(k) * 64 + lane;
        return (j < n) ? widen(pos[j]) : pad_body();
    };
    double4 nxt = (k0 < k1) ? load_chunk(k0) : pad_body();
    for (int k = k0; k < k1; ++k) {
        const double4 cur = nxt;
        if (k + 1 < k1) nxt = load_chunk(k + 1);
        double sj = 0.0;
        // at step s lane l meets the body that started in lane (l - s) & 63, whose running sum it holds
        tile[wv][lane] = cur;   // the wave's own tile: its LDS operations complete in program order
        for (int s = 0; s < 64; ++s) {
            const double4 pj = tile[wv][(lane - s) & 63];
#pragma unroll
            for (int q = 0; q < IPT; ++q) {
                const double inv = inv_dist(pj, xi[q], yi[q], zi[q], eps2);
                si[q] += pj.w * inv;
                sj += mi[q] * inv;
            }
            sj = rot64(sj, src1);
        }
        const int d = k / IPT + 1;   // set distance 1..sym_sets
        planes[size_t(d - 1) * plane_stride + size_t(chunk_of(k)) * 64 + lane] = sj;
    }
    double* __restrict__ out = planes + size_t(sym_sets + part) * plane_stride;
#pragma unroll
    for (int q = 0; q < IPT; ++q) out[size_t(a * IPT + q) * 64 + lane] = si[q];
}

// 4 waves per workgroup; wave gw = group * K + slice: bodies group*64 + lane of the own block against slice `slice` of the
// partner list.  Output: plane `slice`, rows group*64 .. group*64+63 (every row, padding included).
template <class P, int MODE>
__global__ __launch_bounds__(256) void k_pot_os(const P* __restrict__ pos_all, const int* __restrict__ seg_count, int n_seg, int seg_cap,
                                                int my_seg, int set_size, int A, int groups, int K, double* __restrict__ planes,
                                                size_t plane_stride, double eps2) {
    __shared__ double4 tile[4][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wv;
    if (gw >= groups * K) return;
    const int group = gw / K, slice = gw - group * K;
    const int n_own = seg_count[my_seg];
    const int i = group * 64 + lane;
    const double4 pi = (i < n_own) ? widen(pos_all[size_t(my_seg) * seg_cap + i]) : pad_body();
    const int a = (group * 64) / set_size;       // (MODE 1: the set of all 64 bodies of the group)
    double sum = 0.0;
    stream_partners(
        tile[wv], lane, pos_all, seg_cap, n_windows<MODE>(n_seg, A), [&](int w) { return window<MODE>(w, seg_count, my_seg, n_own, set_size, A, a); },
        slice, K, [&](const double4 pj, int seg, int j) {
            const double term = pj.w * inv_dist(pj, pi.x, pi.y, pi.z, eps2);
            sum += (seg == my_seg && j == i) ? 0.0 : term;   // no i == j term
        });
    planes[size_t(slice) * plane_stride + i] = sum;
}

__global__ __launch_bounds__(256) void k_pot_pairs_reduce(const double* __restrict__ planes, int n_planes, size_t plane_stride,
                                                          const int* __restrict__ count, double* __restrict__ sum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *count) return;
    double s = 0.0;
    for (int p = 0; p < n_planes; ++p) s += planes[size_t(p) * plane_stride + i];
    sum[i] = s;
}

template <class P>
__global__ __launch_bounds__(256) void k_pot_energy(const P* __restrict__ pos, const P* __restrict__ vel, const int* __restrict__ count,
                                                    const double* __restrict__ sum, double* __restrict__ out2) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    double ke = 0.0, pe = 0.0;
    if (i < *count) {
        const double4 p = widen(pos[i]), v = widen(vel[i]);
        ke = 0.5 * p.w * ((v.x * v.x + v.y * v.y) + v.z * v.z);
        pe = p.w * sum[i];
    }
    red[0][tid] = ke; red[1][tid] = pe;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
        __syncthreads();
    }
    if (tid == 0) { out2[2 * blockIdx.x] = red[0][0]; out2[2 * blockIdx.x + 1] = red[1][0]; }
}

__global__ __launch_bounds__(256) void k_pot_pack(const int* __restrict__ ids, const double* __restrict__ sum, const int* __restrict__ count,
                                                  PotRec* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < *count) out[i] = PotRec{ids[i], 0, sum[i]};
}

__global__ __launch_bounds__(256) void k_pot_slots(const int* __restrict__ own_ids, const int* __restrict__ own_count, int* __restrict__ slot_of, int n_ids) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= *own_count) return;
    const int id = own_ids[i];
    if (unsigned(id) < unsigned(n_ids)) slot_of[id] = i;
}

// grid.y = rank; every body of the world is in exactly one rank's records, so every own row is written once
__global__ __launch_bounds__(256) void k_pot_scatter(const int* __restrict__ slot_of, int n_ids, const PotRec* __restrict__ rec,
                                                     const int* __restrict__ rec_count, int seg_cap, double* __restrict__ sum) {
    const int r = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= min(rec_count[r], seg_cap)) return;
    const PotRec x = rec[size_t(r) * seg_cap + j];
    if (unsigned(x.id) >= unsigned(n_ids)) return;
    const int slot = slot_of[x.id];
    if (slot >= 0) sum[slot] = x.sum;
}

inline int blocks4(long long waves) { return int((waves + 3) / 4); }

template <class P>
void pairs_impl(hipStream_t s, const PotBodies& b, const nbody64::Bf64Plan& p, double* planes, double eps2, int n_upper, double* sum) {
    const P* pos_all = static_cast<const P*>(b.pos_all);
    const P* own = pos_all + size_t(b.my_seg) * b.seg_cap;
    const int* count = b.seg_count + b.my_seg;
    const dim3 block(256);
    if (p.sym && p.sym_sets > 0) {
        const dim3 grid(blocks4((long long)p.A * p.K));
        if (p.ipt == 4) hipLaunchKernelGGL((k_pot_sym<P, 4>), grid, block, 0, s, own, count, p.A, p.K, p.sym_sets, planes, p.n_pad, eps2);
        else hipLaunchKernelGGL((k_pot_sym<P, 8>), grid, block, 0, s, own, count, p.A, p.K, p.sym_sets, planes, p.n_pad, eps2);
    }
    double* own_out = planes + size_t(p.sym_sets + p.K) * p.n_pad;
    const dim3 og(blocks4((long long)p.groups * p.k_own));
    if (p.sym)
        hipLaunchKernelGGL((k_pot_os<P, 1>), og, block, 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, b.my_seg, 64 * p.ipt, p.A, p.groups, p.k_own,
                           own_out, p.n_pad, eps2);
    else
        hipLaunchKernelGGL((k_pot_os<P, 0>), og, block, 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap, b.my_seg, 64, 1, p.groups, p.k_own,
                           own_out, p.n_pad, eps2);
    if (p.k_remote > 0 && b.n_seg > 1)
        hipLaunchKernelGGL((k_pot_os<P, 2>), dim3(blocks4((long long)p.groups * p.k_remote)), block, 0, s, pos_all, b.seg_count, b.n_seg, b.seg_cap,
                           b.my_seg, 64, 1, p.groups, p.k_remote, own_out + size_t(p.k_own) * p.n_pad, p.n_pad, eps2);
    hipLaunchKernelGGL(k_pot_pairs_reduce, dim3((n_upper + 255) / 256), block, 0, s, planes, p.n_planes, p.n_pad, count, sum);
}

}  // namespace

void launch_pot_pairs(hipStream_t s, const PotBodies& b, const nbody64::Bf64Plan& p, double* planes, double eps2, int n_upper, double* sum) {
    if (n_upper <= 0) return;
    if (b.f64) pairs_impl<double4>(s, b, p, planes, eps2, n_upper, sum);
    else pairs_impl<float4>(s, b, p, planes, eps2, n_upper, sum);
}

void launch_pot_pack(hipStream_t s, const int* ids, const double* sum, const int* count, int n_upper, PotRec* out) {
    if (n_upper <= 0) return;
    hipLaunchKernelGGL(k_pot_pack, dim3((n_upper + 255) / 256), dim3(256), 0, s, ids, sum, count, out);
}

void launch_pot_scatter(hipStream_t s, const int* own_ids, const int* own_count, int own_upper, int* slot_of, int n_ids, const PotRec* rec,
                        const int* rec_count, int world, int seg_cap, double* sum) {
    if (own_upper <= 0 || seg_cap <= 0) return;
    hipLaunchKernelGGL(k_pot_slots, dim3((own_upper + 255) / 256), dim3(256), 0, s, own_ids, own_count, slot_of, n_ids);
    hipLaunchKernelGGL(k_pot_scatter, dim3((seg_cap + 255) / 256, world), dim3(256), 0, s, slot_of, n_ids, rec, rec_count, seg_cap, sum);
}

void launch_pot_energy(hipStream_t s, const PotBodies& b, const double* sum, int n_upper, double* out2) {
    if (n_upper <= 0) return;
    const dim3 grid((n_upper + 255) / 256), block(256);
    const int* count = b.seg_count + b.my_seg;
    if (b.f64)
        hipLaunchKernelGGL(k_pot_energy<double4>, grid, block, 0, s, static_cast<const double4*>(b.pos_all) + size_t(b.my_seg) * b.seg_cap,
                           static_cast<const double4*>(b.vel), count, sum, out2);
    else
        hipLaunchKernelGGL(k_pot_energy<float4>, grid, block, 0, s, static_cast<const float4*>(b.pos_all) + size_t(b.my_seg) * b.seg_cap,
                           static_cast<const float4*>(b.vel), count, sum, out2);
}

}  // namespace nbody

// kernels_quad.hip -- quadrupole moments for the fast f32 Barnes-Hut force walk (nbody_set_multipole) and for
// the tree potentials and the field at caller-chosen points (NBODY_POTENTIAL_TREE_QUADRUPOLE).
//
// k_tree_quad fills a side array with every node's traceless quadrupole tensor about its stored f32 centre of mass c,
//     Q = sum_l m_l (3 d_l d_l^T - |d_l|^2 I),   d_l = c_l - c,
// over the leaves l of its subtree, which in the pre-order array is the index range (i, skip[i]) -- so the same code
// serves the host-built and the device-built tree, and the 32-byte node record and every kernel that reads it stay as
// they are.  k_bh_walk_quad is k_bh_walk<FAST = true, DIRECT> (kernels_bh.hip) with one more term per accepted INTERNAL
// node.  With d = c - x, q = |d|^2 + eps2, inv = 1 / sqrt(q):
//     a += g [ M inv^3 d  -  inv^5 (Q d)  +  2.5 inv^7 (d^T Q d) d ]
// (the gradient of phi = -g [M inv + 1/2 d^T Q d inv^5]).  The opening tests are the oracle's f32 expressions, untouched,
// so {accepted, visited} equal the monopole walk's on the same tree.  The tensor is a second dependent gather, issued
// only after the opening test has accepted an internal node: opened nodes and leaves never touch the side array.
// k_bh_pot_walk_quad and k_bh_field_walk_quad are kernels_bh.hip's k_bh_pot_walk<double> and k_bh_probe_walk with the same
// term (and its scalar counterpart) in IEEE f32 arithmetic: see pot_quad_parts below.
#include "kernels_quad.h"
#include "walk_common.h"

namespace nbody {

constexpr int kQuadWalkBlock = 64;   // as k_bh_walk: one wave per workgroup when the node range is split

struct alignas(32) QuadDev { float4 a; float4 b; };   // {xx, xy, xz, yy}, {yz, zz, 0, 0}

// ---- the tensors
constexpr int kQuadBlock = 256;    // nodes (= threads) per workgroup
constexpr int kQuadSerial = 64;    // a node with at most this many descendants is summed by its own thread

struct Sum6 {
    double xx = 0., xy = 0., xz = 0., yy = 0., yz = 0., zz = 0.;
    // the term of node j about c if j is a leaf (an internal node's leaves follow it in the range)
    __device__ __forceinline__ void add_leaf(const NodeDev* __restrict__ nodes, int j, double cx, double cy, double cz) {
        const float4 A = nodes[j].a;
        if (__float_as_int(nodes[j].b.y) != j + 1) return;
        const double dx = double(A.x) - cx, dy = double(A.y) - cy, dz = double(A.z) - cz, m = double(A.w);   // exact differences
        const double d2 = dx * dx + dy * dy + dz * dz;
        xx += m * (3.0 * dx * dx - d2); yy += m * (3.0 * dy * dy - d2); zz += m * (3.0 * dz * dz - d2);
        xy += m * (3.0 * dx * dy); xz += m * (3.0 * dx * dz); yz += m * (3.0 * dy * dz);
    }
    __device__ __forceinline__ void wave_reduce() {
        for (int off = 32; off > 0; off >>= 1) {
            xx += __shfl_down(xx, off); xy += __shfl_down(xy, off); xz += __shfl_down(xz, off);
            yy += __shfl_down(yy, off); yz += __shfl_down(yz, off); zz += __shfl_down(zz, off);
        }
    }
    __device__ __forceinline__ void store(QuadDev* __restrict__ q) const {
        q->a = make_float4(float(xx), float(xy), float(xz), float(yy));
        q->b = make_float4(float(yz), float(zz), 0.f, 0.f);
    }
};

// One thread per node.  Small subtrees (most nodes: 2/3 are leaves, and the pre-order neighbours of a small cell read
// the same few sectors) are summed by their own thread; the workgroup then sums each of its large ones together, in a
// fixed order (lane stride, shuffle tree, waves in order): the same bits from run to run.  The root's range is the whole
// array, summed by the 256 threads of workgroup 0 -- the launch lasts as long as that one sum.
__global__ __launch_bounds__(kQuadBlock) void k_tree_quad(const NodeDev* __restrict__ nodes, int n_nodes, QuadDev* __restrict__ quad,
                                                          const int* __restrict__ info, const int* __restrict__ poison) {
    __shared__ int big[kQuadBlock];
    __shared__ int n_big;
    __shared__ double part[kQuadBlock / 64][6];
    if (poison && *poison) return;
    if (info) n_nodes = min(n_nodes, info[0]);
    if (threadIdx.x == 0) n_big = 0;
    __syncthreads();
    const int i = blockIdx.x * kQuadBlock + threadIdx.x;
    if (i < n_nodes) {
        const int end = min(__float_as_int(nodes[i].b.y), n_nodes);   // (a link is never beyond the array; a cheap guard all the same)
        if (end - i - 1 <= kQuadSerial) {
            const float4 C = nodes[i].a;
            Sum6 s;
            for (int j = i + 1; j < end; ++j) s.add_leaf(nodes, j, double(C.x), double(C.y), double(C.z));
            s.store(quad + i);
        } else {
            big[atomicAdd(&n_big, 1)] = i;   // (LDS; the order of the list decides nothing: every entry is summed on its own)
        }
    }
    __syncthreads();
    const int nb = n_big;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < nb; ++k) {
        const int b = big[k];
        const int end = min(__float_as_int(nodes[b].b.y), n_nodes);
        const float4 C = nodes[b].a;
        Sum6 s;
        for (int j = b + 1 + int(threadIdx.x); j < end; j += kQuadBlock) s.add_leaf(nodes, j, double(C.x), double(C.y), double(C.z));
        s.wave_reduce();
        if (lane == 0) { part[wave][0] = s.xx; part[wave][1] = s.xy; part[wave][2] = s.xz; part[wave][3] = s.yy; part[wave][4] = s.yz; part[wave][5] = s.zz; }
        __syncthreads();
        if (threadIdx.x == 0) {
            Sum6 t;
            for (int w = 0; w < kQuadBlock / 64; ++w) { t.xx += part[w][0]; t.xy += part[w][1]; t.xz += part[w][2]; t.yy += part[w][3]; t.yz += part[w][4]; t.zz += part[w][5]; }
            t.store(quad + b);
        }
        __syncthreads();
    }
}

// ---- the walk
struct QuadSplit {           // walk_common.h WalkSplit, what the one-body-per-lane walk reads of it
    int n_seg;
    const int* first;        // [n_seg + 1]
    const int* anc;          // [n_seg][kMaxAnc] ancestors of first[k], root first
    const int* n_anc;        // [n_seg]
    float4* planes;          // [n_seg][plane_stride] partial accelerations by place in the tree order (n_seg > 1)
    size_t plane_stride;
    int diag_first;          // Tuning::bh_walk_order
    const int* poison;       // unsynchronised steps: != 0 -> do nothing; may be null
    const int* n_order_dev;  // unsynchronised steps: the live number of bodies to walk; may be null
};

// walk_common.h walk_entry: the first node >= first[seg] the body's walk visits (the opening tests of first[seg]'s ancestors)
template <bool DIRECT>
__device__ __forceinline__ int quad_walk_entry(const NodeDev* __restrict__ nodes, const QuadSplit& sp, int seg, const float4 p, float theta2) {
    const int na = sp.n_anc[seg];
    for (int k = 0; k < na; ++k) {
        const int j = sp.anc[seg * kMaxAnc + k];
        const float4 A = nodes[j].a;
        const float4 B = nodes[j].b;
        const float rx = A.x - p.x, ry = A.y - p.y, rz = A.z - p.z;
        const float r2 = (rx * rx + ry * ry) + rz * rz;
        if (DIRECT && r2 < 1e-10f) return __float_as_int(B.y);
        if (B.x < theta2 * r2) return __float_as_int(B.y);
    }
    return sp.first[seg];
}

// The term of an accepted node, added to (ax, ay, az).  In u = d inv (|u| <= 1) the three parts are
//     g inv^2 [ M u + inv^2 (2.5 (u^T Q u) u - Q u) ]:
// the same algebra as the definition, and no power of inv beyond the fourth (inv^7 overflows f32 below r ~ 3e-6).
__device__ __forceinline__ void quad_term(const float4 A, const QuadDev* __restrict__ quad, int i, bool internal, float rx, float ry, float rz,
                                          float r2, float g, float eps2, float& ax, float& ay, float& az) {
    const float rinv = __builtin_amdgcn_rsqf(r2 + eps2);
    if (!internal) {   // a leaf: the monopole term as k_bh_walk<FAST> rounds it
        const float k = monopole_k<true, true>(g, A.w, r2, eps2);
        ax += rx * k; ay += ry * k; az += rz * k;
        return;
    }
    const float4 Qa = quad[i].a, Qb = quad[i].b;   // {xx, xy, xz, yy}, {yz, zz}: the second gather, one 32-byte sector
    const float s = g * (rinv * rinv), kq = s * (rinv * rinv);
    const float ux = rx * rinv, uy = ry * rinv, uz = rz * rinv;
    const float qx = __builtin_fmaf(Qa.x, ux, __builtin_fmaf(Qa.y, uy, Qa.z * uz));
    const float qy = __builtin_fmaf(Qa.y, ux, __builtin_fmaf(Qa.w, uy, Qb.x * uz));
    const float qz = __builtin_fmaf(Qa.z, ux, __builtin_fmaf(Qb.x, uy, Qb.y * uz));
    const float uqu = __builtin_fmaf(ux, qx, __builtin_fmaf(uy, qy, uz * qz));
    const float coef = __builtin_fmaf(2.5f * uqu, kq, s * A.w);
    ax = __builtin_fmaf(coef, ux, __builtin_fmaf(-kq, qx, ax));
    ay = __builtin_fmaf(coef, uy, __builtin_fmaf(-kq, qy, ay));
    az = __builtin_fmaf(coef, uz, __builtin_fmaf(-kq, qz, az));
}

template <bool DIRECT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_bh_walk_quad(const NodeDev* __restrict__ nodes, const QuadDev* __restrict__ quad,
                                                        const int* __restrict__ order, int n_order, const float4* __restrict__ own_pos,
                                                        float4* __restrict__ acc, float g, float eps2, float theta2,
                                                        unsigned long long* __restrict__ counters, QuadSplit split) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    int seg = blockIdx.y;
    if (split.diag_first) {   // a body group's segments nearest its own place in the tree first (k_bh_walk)
        seg = nearest_first_segment(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
    }
    if (split.poison && *split.poison) return;
    if (split.n_order_dev) n_order = min(n_order, *split.n_order_dev);
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n_order) {
        const int b = order[t];
        const float4 p = own_pos[b];
        float ax = 0.f, ay = 0.f, az = 0.f;
        int i = quad_walk_entry<DIRECT>(nodes, split, seg, p, theta2);
        while (i < s1) {
            const float4 A = nodes[i].a;
            const float2 B = *reinterpret_cast<const float2*>(&nodes[i].b);   // {w^2, skip link}
            asm volatile("" :: "v"(A.w), "v"(B.y));   // both loads whole and ahead of the branch (k_bh_walk)
            const float rx = A.x - p.x, ry = A.y - p.y, rz = A.z - p.z;
            const float r2 = (rx * rx + ry * ry) + rz * rz;
            const int skip = __float_as_int(B.y);
            const bool leaf = skip == i + 1;
            ++n_vis;
            if (DIRECT && r2 < 1e-10f) { i = skip; continue; }
            if (B.x < theta2 * r2 || (DIRECT && leaf)) {
                quad_term(A, quad, i, !leaf, rx, ry, rz, r2, g, eps2, ax, ay, az);
                ++n_acc;
                i = skip;
            } else {
                i = i + 1;
            }
        }
        *(split.n_seg > 1 ? split.planes + size_t(seg) * split.plane_stride + t : acc + b) = make_float4(ax, ay, az, 0.f);
    }
    add_walk_counts(counters, blockIdx.x + blockIdx.y * gridDim.x, n_acc, n_vis);
}

// ---- NBODY_POTENTIAL_TREE_QUADRUPOLE: the potential walk and the field walk with the term of every accepted internal node.
// A leaf's term is the monopole walk's, rounded as k_bh_pot_walk / k_bh_probe_walk round it.  The quadrupole parts of an
// internal node, operation by operation (every line one f32 rounding, fmaf one; IEEE sqrt and divide; tests/quad_pot_list.py
// counts these roundings for its bounds):
//     q   = r2 + eps2            s = sqrtf(q)            inv = 1.0f / s
//     u_c = d_c * inv                                                            c = x, y, z      (|u| <= 1)
//     p_c = fmaf(Q_c0, u_0, fmaf(Q_c1, u_1, Q_c2 * u_2))                         = (Q u)_c
//     uqu = fmaf(u_0, p_0, fmaf(u_1, p_1, u_2 * p_2))                            = u^T Q u
//     i2  = inv * inv
//   scalar   P   = ((0.5f * uqu) * i2) * inv                                     = 1/2 (d^T Q d) inv^5
//     i4  = i2 * i2              w = (2.5f * uqu) * i4
//   vector   V_c = fmaf(w, u_c, -(i4 * p_c))                                     = 2.5 inv^7 (d^T Q d) d_c - inv^5 (Q d)_c
// The monopole parts of an internal node are k_bh_probe_walk's: st = M * inv, vector d_c * (st / q).  No power of inv beyond
// the fourth: nodes closer than 1e-5 are skipped whole, so inv <= 1e5 and i4 <= 1e20.  A probe so far away that r2 overflows
// has inv = 0, u = 0 (d is finite) and st / q = 0 / inf = 0: every part is an exact zero, never 0 * inf.
struct QuadParts { float P, Vx, Vy, Vz; };

template <bool VEC, bool SCAL>
__device__ __forceinline__ QuadParts pot_quad_parts(const QuadDev* __restrict__ quad, int i, float rx, float ry, float rz, float inv) {
    const float4 Qa = quad[i].a;
    const float2 Qb = *reinterpret_cast<const float2*>(&quad[i].b);   // {xx, xy, xz, yy}, {yz, zz}: the second gather, one 32-byte sector
    const float ux = rx * inv, uy = ry * inv, uz = rz * inv;
    const float px = __builtin_fmaf(Qa.x, ux, __builtin_fmaf(Qa.y, uy, Qa.z * uz));
    const float py = __builtin_fmaf(Qa.y, ux, __builtin_fmaf(Qa.w, uy, Qb.x * uz));
    const float pz = __builtin_fmaf(Qa.z, ux, __builtin_fmaf(Qb.x, uy, Qb.y * uz));
    const float uqu = __builtin_fmaf(ux, px, __builtin_fmaf(uy, py, uz * pz));
    const float i2 = inv * inv;
    QuadParts r{0.f, 0.f, 0.f, 0.f};
    if (SCAL) r.P = ((0.5f * uqu) * i2) * inv;
    if (VEC) {
        const float i4 = i2 * i2;
        const float w = (2.5f * uqu) * i4;
        r.Vx = __builtin_fmaf(w, ux, -(i4 * px));
        r.Vy = __builtin_fmaf(w, uy, -(i4 * py));
        r.Vz = __builtin_fmaf(w, uz, -(i4 * pz));
    }
    return r;
}

// k_bh_pot_walk<double> (kernels_bh.hip) with the scalar quadrupole part: the same tests, planes and counter slots
__global__ __launch_bounds__(kQuadWalkBlock) void k_bh_pot_walk_quad(const NodeDev* __restrict__ nodes, const QuadDev* __restrict__ quad,
                                                                     const int* __restrict__ order, int n_order, const float4* __restrict__ own_pos,
                                                                     float eps2, float theta2, unsigned long long* __restrict__ counters,
                                                                     QuadSplit split, double* __restrict__ planes, size_t plane_stride) {
    const int t = blockIdx.x * kQuadWalkBlock + threadIdx.x;
    if (split.n_order_dev) n_order = min(n_order, *split.n_order_dev);
    const int seg = nearest_first_segment(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);   // (as k_bh_walk dispatches them)
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n_order) {
        const float4 p = own_pos[order[t]];
        double sum = 0.0;
        int i = quad_walk_entry<true>(nodes, split, seg, p, theta2);
        while (i < s1) {
            const float4 A = nodes[i].a;
            const float2 B = *reinterpret_cast<const float2*>(&nodes[i].b);
            asm volatile("" :: "v"(A.w), "v"(B.y));   // (both loads whole and ahead of the branches: see k_bh_walk)
            const float rx = A.x - p.x, ry = A.y - p.y, rz = A.z - p.z;
            const float r2 = (rx * rx + ry * ry) + rz * rz;
            const int skip = __float_as_int(B.y);
            const bool leaf = skip == i + 1;
            ++n_vis;
            if (r2 < 1e-10f) { i = skip; continue; }                  // skipped whole (how a body skips itself)
            if (leaf) {                                                // evaluated whether it passes the test or not: k_bh_pot_walk's term
                sum += double(A.w / __builtin_sqrtf(r2 + eps2));
                ++n_acc;
                i = skip;
            } else if (B.x < theta2 * r2) {                            // accepted cell
                const float inv = 1.0f / __builtin_sqrtf(r2 + eps2);
                sum += double(A.w * inv);
                sum += double(pot_quad_parts<false, true>(quad, i, rx, ry, rz, inv).P);
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

// k_bh_probe_walk<FieldTerm<VEC, SCAL>> (kernels_bh.hip) with both quadrupole parts
template <bool VEC, bool SCAL>
__global__ __launch_bounds__(kQuadWalkBlock) void k_bh_field_walk_quad(const NodeDev* __restrict__ nodes, const QuadDev* __restrict__ quad,
                                                                       const double* __restrict__ xyz, const int* __restrict__ idx, int n,
                                                                       float eps2, float theta2, unsigned long long* __restrict__ counters,
                                                                       QuadSplit split, double4* __restrict__ planes, size_t plane_stride) {
    const int t = blockIdx.x * kQuadWalkBlock + threadIdx.x;
    const int seg = nearest_first_segment(blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);   // (as k_bh_walk dispatches them)
    const int s1 = split.first[seg + 1];
    unsigned int n_acc = 0, n_vis = 0;
    if (t < n) {
        const size_t c = size_t(idx[t]);
        const float4 p = make_float4(float(xyz[3 * c]), float(xyz[3 * c + 1]), float(xyz[3 * c + 2]), 0.f);
        const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
        double ax = 0.0, ay = 0.0, az = 0.0, sum = 0.0;
        int i = quad_walk_entry<true>(nodes, split, seg, p, theta2);
        while (i < s1) {
            const float4 A = nodes[i].a;
            const float2 B = *reinterpret_cast<const float2*>(&nodes[i].b);
            asm volatile("" :: "v"(A.w), "v"(B.y));   // (both loads whole and ahead of the branches: see k_bh_walk)
            const float rx = A.x - p.x, ry = A.y - p.y, rz = A.z - p.z;
            const float r2 = (rx * rx + ry * ry) + rz * rz;
            const int skip = __float_as_int(B.y);
            const bool leaf = skip == i + 1;
            ++n_vis;
            if (r2 < 1e-10f) { i = skip; continue; }                  // skipped whole (a probe on a body skips it)
            if (B.x < theta2 * r2 || leaf) {                           // accepted cell, or a leaf that failed the test
                const float q = r2 + eps2;
                const float inv = 1.0f / __builtin_sqrtf(q);
                const float st = A.w * inv;
                if (SCAL) sum += double(st);
                if (VEC) {
                    const float k = st / q;
                    ax += double(rx * k); ay += double(ry * k); az += double(rz * k);
                }
                if (!leaf && (VEC || SCAL)) {
                    const QuadParts qp = pot_quad_parts<VEC, SCAL>(quad, i, rx, ry, rz, inv);
                    if (SCAL) sum += double(qp.P);
                    if (VEC) { ax += double(qp.Vx); ay += double(qp.Vy); az += double(qp.Vz); }
                }
                ++n_acc;
                i = skip;
            } else {
                i = i + 1;
            }
        }
        if (VEC || SCAL) {
            const double bad = __longlong_as_double(0x7ff8000000000000ll);
            planes[size_t(seg) * plane_stride + t] = finite ? make_double4(ax, ay, az, sum) : make_double4(bad, bad, bad, bad);
        }
    }
    add_walk_counts(counters, blockIdx.x + blockIdx.y * gridDim.x, n_acc, n_vis);
}

void launch_tree_quad(hipStream_t s, const float4* nodes, int n_nodes, float4* quad, const int* info, const int* poison) {
    if (n_nodes <= 0) return;
    hipLaunchKernelGGL(k_tree_quad, dim3((n_nodes + kQuadBlock - 1) / kQuadBlock), dim3(kQuadBlock), 0, s, reinterpret_cast<const NodeDev*>(nodes),
                       n_nodes, reinterpret_cast<QuadDev*>(quad), info, poison);
}

void launch_bh_walk_quad(hipStream_t s, const Shard& sh, const TreeDev& t, const float4* quad, float g, float g_soft2, float theta2,
                         unsigned long long* counters, int leaf_direct, const float* kick_dt, int* kicked) {
    if (kicked) *kicked = 0;
    if (t.n_order <= 0) return;
    QuadSplit sp;
    sp.n_seg = t.n_split; sp.first = t.split_first; sp.anc = t.split_anc; sp.n_anc = t.split_n_anc;
    sp.planes = t.split_planes; sp.plane_stride = t.split_stride;
    sp.diag_first = tuning().bh_walk_order;
    sp.poison = t.poison; sp.n_order_dev = t.n_order_dev;
#define WALKQ(DIRECT, BLK) hipLaunchKernelGGL((k_bh_walk_quad<DIRECT, BLK>), dim3((t.n_order + BLK - 1) / BLK, t.n_split), dim3(BLK), 0, s, \
                                              reinterpret_cast<const NodeDev*>(t.nodes), reinterpret_cast<const QuadDev*>(quad), t.order, t.n_order, sh.own_pos(), sh.acc, g, g_soft2, theta2, counters, sp)
    if (t.n_split <= 2) { if (leaf_direct) WALKQ(true, 256); else WALKQ(false, 256); }   // (k_bh_walk's rule: enough bodies to fill the chip)
    else { if (leaf_direct) WALKQ(true, kQuadWalkBlock); else WALKQ(false, kQuadWalkBlock); }
#undef WALKQ
    launch_bh_reduce(s, sh, t, 1, kick_dt, kicked);
}

void launch_bh_pot_walk_quad(hipStream_t s, const float4* own_pos, const TreeDev& t, const float4* quad, float g_soft2, float theta2,
                             double* planes, size_t plane_stride, double* sum, unsigned long long* counters) {
    if (t.n_order <= 0) return;
    QuadSplit sp{};
    sp.n_seg = t.n_split; sp.first = t.split_first; sp.anc = t.split_anc; sp.n_anc = t.split_n_anc;
    sp.n_order_dev = t.n_order_dev;
    hipLaunchKernelGGL(k_bh_pot_walk_quad, dim3((t.n_order + kQuadWalkBlock - 1) / kQuadWalkBlock, t.n_split), dim3(kQuadWalkBlock), 0, s,
                       reinterpret_cast<const NodeDev*>(t.nodes), reinterpret_cast<const QuadDev*>(quad), t.order, t.n_order, own_pos, g_soft2, theta2,
                       counters, sp, planes, plane_stride);
    launch_pot_reduce(s, planes, t.n_split, plane_stride, t.order, t.n_order, sum, t.n_order_dev);
}

void launch_bh_field_walk_quad(hipStream_t s, const FieldTree& t, const float4* quad, const double* xyz, const int* idx, int n, float eps2,
                               float theta2, int want, double4* planes, size_t stride, unsigned long long* counters) {
    if (n <= 0) return;
    QuadSplit sp{};
    sp.n_seg = t.K; sp.first = t.first; sp.anc = t.anc; sp.n_anc = t.n_anc;
    const dim3 grid((n + kQuadWalkBlock - 1) / kQuadWalkBlock, t.K);
    const NodeDev* nodes = static_cast<const NodeDev*>(t.nodes);
    const QuadDev* qd = reinterpret_cast<const QuadDev*>(quad);
#define FIELD_WALKQ(V, S) hipLaunchKernelGGL((k_bh_field_walk_quad<V, S>), grid, dim3(kQuadWalkBlock), 0, s, nodes, qd, xyz, idx, n, eps2, theta2, counters, sp, planes, stride)
    if (want == 3) FIELD_WALKQ(true, true); else if (want == 1) FIELD_WALKQ(true, false); else if (want == 2) FIELD_WALKQ(false, true); else FIELD_WALKQ(false, false);
#undef FIELD_WALKQ
}

}  // namespace nbody

// retain.h -- the one copy of the look-back retain that k_compact (f32 and f64, kernels_integrate.hip) and k_hm_compact
// (kernels_hermite.hip) wrap.  Device code only.
//
// K4: Vec::retain (brute_force.rs:86, barnes_hut.rs:267) -- order-preserving compaction of the own segment, in
// place, in ONE pass over many workgroups (round 1 walked the segment with a single 1 024-thread workgroup: an escape
// at N = 2^22 serialised 4 096 chunk iterations on one CU, ms-scale).  Launched every step, every workgroup returns at
// once unless drift_half flagged an escape.
//   * a tile = 1 024 consecutive bodies, one per thread; the thread loads its record, the workgroup counts and ranks
//     its survivors (wave ballots + 16 wave totals in LDS);
//   * tiles learn how many survivors precede them by decoupled look-back: a tile publishes {its own count}, then adds
//     up its predecessors' published counts backwards until it meets one that already knows its inclusive prefix, and
//     publishes its own inclusive prefix.  Status words carry the launch's epoch, so they never need resetting;
//   * in place: a survivor moves to an index <= its own, i.e. into the source range of its own or an EARLIER tile.  A
//     tile publishes only after its own records are in registers, and a tile's prefix is built from published words
//     only, so -- by induction over the tiles it looked back over -- every earlier tile has finished reading before
//     this tile knows where to write; inside a tile a barrier separates the loads from the stores.
#pragma once
#include <hip/hip_runtime.h>

namespace nbody {

constexpr int kCompactTile = 1024;
constexpr unsigned long long kTileAgg = 1ull, kTilePrefix = 2ull;
__device__ __forceinline__ unsigned long long tile_word(int epoch, unsigned long long flag, int value) {
    return ((unsigned long long)(unsigned)epoch << 34) | (flag << 32) | (unsigned long long)(unsigned)value;
}

// One tile of the retain, called by every thread of a kCompactTile-thread workgroup (blockIdx.x = the tile) after the
// kernel's early-outs.  What moves with a body is the caller's: `load(k)` takes body k into the caller's registers, `store(d)`
// writes them to index d.  The core calls both itself, for the survivors only, the load before anything is published and
// the store after the tile knows its prefix -- the order the argument above rests on.
// tile_state: [ceil(capacity / kCompactTile) + 1] words, zeroed once when allocated; *epoch_p: the launch's epoch.
template <class Load, class Store>
__device__ __forceinline__ void retain_tile(const unsigned char* __restrict__ keep, int* __restrict__ count, int* __restrict__ escaped,
                                            unsigned long long* __restrict__ tile_state, int* __restrict__ epoch_p, Load load,
                                            Store store) {
    __shared__ int wave_total[kCompactTile / 64];
    __shared__ int excl_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x;
    const int n = *count;
    const int epoch = *epoch_p & 0x3fffffff;
    const int k = tile * kCompactTile + tid;
    const bool kp = (k < n) && keep[k];
    if (kp) load(k);
    const unsigned long long m = __ballot(kp);
    const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[wave] = __popcll(m);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's records are in registers ...
    __syncthreads();                                   // ... and so are the whole tile's
    int before = 0, total = 0;
    for (int w = 0; w < kCompactTile / 64; ++w) {
        const int t = wave_total[w];
        if (w < wave) before += t;
        total += t;
    }
    if (tid == 0) {
        volatile unsigned long long* st = tile_state;
        int excl = 0;
        if (tile == 0) {
            st[0] = tile_word(epoch, kTilePrefix, total);
        } else {
            st[tile] = tile_word(epoch, kTileAgg, total);
            __threadfence();
            for (int j = tile - 1; j >= 0;) {
                const unsigned long long wd = st[j];
                if (int(wd >> 34) != epoch) continue;            // not published in this launch yet: look again
                excl += int(unsigned(wd & 0xFFFFFFFFull));
                if (((wd >> 32) & 3ull) == kTilePrefix) break;   // everything before j is in this word
                --j;
            }
            st[tile] = tile_word(epoch, kTilePrefix, excl + total);
        }
        __threadfence();
        excl_s = excl;
        if (tile == int(gridDim.x) - 1) {   // the last tile's inclusive prefix is the new body count
            *count = excl + total;
            *escaped = 0;
            *epoch_p = (epoch + 1) & 0x3fffffff;
        }
    }
    __syncthreads();
    if (kp) store(excl_s + before + in_wave);
}

}  // namespace nbody

// shard.h -- the device-resident body state of one shard, once for F = f32 and F = f64, and the part of real.h that host
// code needs for it (the vector and bounds types of F).  Included by kernels.h and kernels_f64.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace nbody64 {
struct Bounds64 { double lo[3]; double hi[3]; };   // Bounds::min()/max() (shared.rs:223-229) evaluated on the host in f64
}
namespace nbody {

struct BoundsF {  // Bounds::min()/max() (shared.rs:223-229) evaluated once on the host in f32
    float lo[3];
    float hi[3];
};

// the types of F that host and device code share (real.h's Real<F> adds the device arithmetic).  The two bounds records
// keep their names: kernels take them by value, and a kernel's symbol carries its parameter types.
template <class F> struct RealTypes;
template <> struct RealTypes<float> { using V4 = float4; using Bounds = BoundsF; };
template <> struct RealTypes<double> { using V4 = double4; using Bounds = nbody64::Bounds64; };

// Device-resident body state of one shard.  Positions of ALL shards live in `pos_all`
// (world_size segments of `seg_cap` V4 {x,y,z,m}, refreshed by the per-step exchange); velocities and accelerations only
// for the shard's own segment.  Body counts are device-resident so that bodies can leave the box
// (Vec::retain, brute_force.rs:86) without a host round trip.
template <class F>
struct ShardT {
    using V4 = typename RealTypes<F>::V4;
    V4* pos_all = nullptr;       // [n_seg * seg_cap]  {x, y, z, mass}
    V4* vel = nullptr;           // [seg_cap]          {vx, vy, vz, 0}
    V4* acc = nullptr;           // [seg_cap]          {ax, ay, az, 0}
    int* seg_count = nullptr;    // [n_seg] bodies alive per segment
    int* escaped = nullptr;      // [1] bodies of the own segment flagged out of bounds by drift
    unsigned char* keep = nullptr;  // [seg_cap] 1 = in bounds
    // K4 (parallel retain, retain.h): per-tile status words of the decoupled look-back {epoch | flag | count} and the epoch
    unsigned long long* tile_state = nullptr;   // [ceil(seg_cap / 1024) + 1]
    int* epoch = nullptr;                       // [1]
    // Barnes-Hut steps enqueued without a host round trip (device tree): [0] != 0 = "poisoned" (a build needed the
    // host: deeper than the device build's 21 levels, or more nodes than allocated) -- every kernel that changes the
    // state then does nothing until the host has dealt with it; [1] = steps completed since the host last looked.
    // Null on f64 handles.
    int* poison = nullptr;
    int* ids = nullptr;                         // [seg_cap] spatial shards: index of each own body in the uploaded vector (moves with it); else null
    unsigned long long* inter = nullptr;        // [1] brute force: directed interactions evaluated, n_own * (n_total - 1) per force pass from the LIVE counts
    int n_seg = 1;
    int seg_cap = 0;
    int my_seg = 0;
    V4* own_pos() const { return pos_all + size_t(my_seg) * seg_cap; }
    int* own_count() const { return seg_count + my_seg; }
};
using Shard = ShardT<float>;

}  // namespace nbody
namespace nbody64 { using Dev = nbody::ShardT<double>; }

// kernels_unbind.h -- launchers of the iterative unbinding of friends-of-friends groups (kernels_unbind.hip): per-member
// energies restricted to the member's own group, the verdict that strips the unbound members of a pass at once, and the
// compaction of what is left (include/nbody_hip.h, "self-bound subsets of friends-of-friends groups").  They work on the
// catalogue and the member list that launch_catalogue (kernels_fof.h) left in a FofScratch.  Internal to libnbody_hip.so.
#pragma once
#include "kernels_fof.h"

namespace nbody { namespace fof {

// the state of one listed FoF group across the passes
struct UnbindGroup {
    int running;      // 1 while the group takes part in the next pass
    int iterations;   // passes it went through
    int converged;    // 1: its last pass found nobody unbound
    int alive;        // members whose flag is set; < min_members: dissolved
    double sum[7];    // mass, m x, m v of the alive members at its last pass
};

// The scratch of the passes for n_members listed members in n_groups listed groups, carved out of one allocation.
struct UnbindScratch {
    UnbindGroup* grp = nullptr;         // [n_groups]
    int* alive = nullptr;               // [n_members] parallel to the FoF member list: 1 = still a member
    int* mark = nullptr;                // [n_members] during the passes: 1 = unbound in this pass; at the end: 1 = reported
    int* dest = nullptr;                // [n_members] exclusive prefix sums of mark: the member's place in the reported list
    double* energy = nullptr;           // [n_members] e_i of the member's last pass
    double* kinetic = nullptr;          // [n_members] (0.5 m_i) u2_i
    double* potential = nullptr;        // [n_members] (0.5 m_i) phi_i
    int* keep = nullptr;                // [n_groups] 1 = reported
    int* kept = nullptr;                // [n_groups] alive where keep, else 0
    int* slot = nullptr;                // [n_groups] exclusive prefix sums of keep
    int* offset = nullptr;              // [n_groups] exclusive prefix sums of kept
    int* out_members = nullptr;         // [n_members] the reported members
    double* out_energy = nullptr;       // [n_members] parallel to out_members
    NbodyBoundGroup* out = nullptr;     // [n_groups] the reported records
    int* counters = nullptr;            // [3] groups still running after a pass | reported groups | reported members
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
};
size_t unbind_scratch_bytes(size_t n_members, size_t n_groups);
UnbindScratch unbind_layout(void* base, size_t n_members, size_t n_groups);

// k_unbind_init: every flag 1, every group running with all its members
void launch_unbind_init(hipStream_t s, int n_members, int n_groups, const FofScratch& w, const UnbindScratch& u);

// One evaluation pass over the groups still running: k_unbind_sums<F> (one wave per group), k_unbind_energy<F> (one member per
// lane, n_members / 256 blocks) and k_unbind_verdict (one wave per group), which sets iterations = pass + 1, stops the groups
// with nobody unbound and, on the last pass, everybody; else strips the unbound and counts the groups that go on in
// u.counters[0] (zeroed by the caller before the pass).
template <class F>
void launch_unbind_pass(hipStream_t s, const ShardT<F>& sh, int n_upper, int n_members, int n_groups, int min_members, int pass,
                        bool last, double g, double soft2, const FofScratch& w, const UnbindScratch& u);

// After the last pass: the reported groups and members compacted in order (flags, two integer scans over the groups, one over
// the members), u.out, u.out_members, u.out_energy and u.counters[1 .. 2].  Returns 0, or -1 when a rocPRIM call could not be
// enqueued.
int launch_unbind_finish(hipStream_t s, int n_upper, int n_members, int n_groups, int min_members, const FofScratch& w,
                         const UnbindScratch& u);

}}  // namespace nbody::fof

// kernels_pairs.h -- launchers of the binary census (kernels_pairs.hip): every body's partner of least two-body energy, the
// mutual bound pairs among them and their orbital elements; and of the sticky mergers on the same frame: every body's nearest
// neighbour, the mutual contacts within a radius and their merged records.  Internal to libnbody_hip.so.
#pragma once
#include "nbody_hip.h"   // NbodyBoundPair, NbodyContact
#include "shard.h"

namespace nbody { namespace pairs {

constexpr int kPairBlock = 256;   // bodies per block of k_partner, and partners per LDS tile

inline int blocks_for(int n) { return n <= 0 ? 0 : (n + kPairBlock - 1) / kPairBlock; }

// the temporary storage of rocprim::exclusive_scan over n ints with plus<int>: the scan of every query's flags and counts
size_t scan_tmp_bytes(size_t n);

// k_partner's grid for n_upper >= live bodies: groups of kPairBlock bodies x K partner slices, about bf64_waves waves in all
// (make_hm_act_plan's rule: a slice holds 64 partners or more); slice s of n live bodies is [n s / K, n (s + 1) / K)
struct PartnerPlan { int groups = 0, K = 1; };
PartnerPlan make_partner_plan(int n_upper);
// the same rule for n_upper bodies against `partners` partners that are not the bodies themselves (k_pair_hist's cross form)
PartnerPlan make_partner_plan(int n_upper, int partners);

// The scratch of one call for n_upper rows, carved out of one allocation of scratch_bytes.
struct PairScratch {
    double* rec_e = nullptr;          // [K][groups * kPairBlock] the least energy of (slice, body)
    int* rec_j = nullptr;             // [K][groups * kPairBlock] and its partner (-1: none)
    double* energy = nullptr;         // [n_upper] the least energy of a body, +inf: none (launch_nearest: the least r2)
    int* partner = nullptr;           // [n_upper] its partner, -1: none (launch_nearest: the nearest body)
    int* flag = nullptr;              // [n_upper] 1 = the first body of a mutual bound pair (launch_contacts: of a contact)
    int* offset = nullptr;            // [n_upper] exclusive prefix sums of flag
    int* total = nullptr;             // [1] pairs
    NbodyBoundPair* pairs = nullptr;  // [n_upper / 2 + 1]
    NbodyContact* contacts = nullptr; // [n_upper / 2 + 1] the same block: a call lists bound pairs or contacts
    void* scan_tmp = nullptr;
    size_t scan_bytes = 0;
};
size_t scratch_bytes(size_t n_upper, const PartnerPlan& p, bool want_pairs);
PairScratch scratch_layout(void* base, size_t n_upper, const PartnerPlan& p, bool want_pairs);

// k_partner and k_partner_merge: w.partner and w.energy of the live bodies (rows past the live count: -1 and +inf)
template <class F>
void launch_partners(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, double g, double soft2, const PairScratch& w);

// k_pair_flag, the integer scan, k_pair_emit: w.pairs in ascending first index and *w.total of them, from w.partner and
// w.energy.  Returns 0, or -1 when the scan could not be enqueued.
template <class F>
int launch_bound_pairs(hipStream_t s, const ShardT<F>& sh, int n_upper, double g, const PairScratch& w);

// ---- sticky mergers: the metric is r2 = (dx dx + dy dy) + dz dz, unsoftened
// k_partner<F, kDist> and k_partner_merge: w.partner = every live body's nearest body, w.energy = its r2
template <class F>
void launch_nearest(hipStream_t s, const ShardT<F>& sh, int n_upper, const PartnerPlan& p, const PairScratch& w);
// k_contact_flag (mutual, j > i, r2 < R2), the integer scan, k_contact_emit<F, false>: w.contacts in ascending i (`into` 0:
// the host fills it) and *w.total of them.  Writes nothing of sh.  Returns 0, or -1 when the scan could not be enqueued.
template <class F>
int launch_contacts(hipStream_t s, const ShardT<F>& sh, int n_upper, double R2, const PairScratch& w);
// k_contact_emit<F, true> after launch_contacts: the merged record into row i of pos, vel, acc (and jerk, unless null), the
// keep flags of every live row (0 for the absorbed j) and *sh.escaped raised -- what the retain (launch_compact /
// launch_hm_compact) that the caller enqueues next needs.  Call it only when *w.total > 0.
template <class F>
void launch_merge(hipStream_t s, const ShardT<F>& sh, typename ShardT<F>::V4* jerk, int n_upper, const PairScratch& w);

}}  // namespace nbody::pairs

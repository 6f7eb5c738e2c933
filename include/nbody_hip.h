/* nbody_hip.h -- C ABI of the MI355X (gfx950) N-body force-and-integrate engine.
 *
 * The reference (alxn3/nbody-llm) has no FFI for this path: its operator interface is the Rust
 * trait `Simulation<F, D, P, I>` (src/shared.rs:80-97) implemented by
 * `BruteForceSimulation` (src/manual/brute_force.rs:28-103) and `BarnesHutSimulation`
 * (src/manual/barnes_hut.rs:205-285).  Every entry point below names the trait method (or
 * reference function) it stands in for; INTEGRATION.md shows the Rust `extern "C"` block and the
 * `impl Simulation` a maintainer would add on the reference side.
 *
 * Conventions
 *   - every call returns int: 0 = NBODY_OK, < 0 = error (nbody_last_error() has the text);
 *     no exception or panic crosses the boundary;
 *   - a handle is used from one thread at a time (the reference calls its simulation from one
 *     thread: src/main.rs:119-122, src/vis.rs:537-553);
 *   - the library owns all device memory; host buffers are caller-owned and only touched
 *     during the call;
 *   - bodies cross the boundary as `PointParticle<F,3>` records (src/shared.rs:151-158,
 *     #[repr(C)]): 10 scalars {pos[3], vel[3], acc[3], mass} -- F = f32: 40 bytes (NbodyConfig.dtype =
 *     NBODY_F32), F = f64: 80 bytes (NBODY_F64; the reference's own driver runs f64, src/main.rs:52-105);
 *   - there is no CPU fallback: without a HIP device nbody_create fails with NBODY_ERR_NO_DEVICE.
 */
#ifndef NBODY_HIP_H
#define NBODY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_ABI_VERSION 4

typedef struct NbodyHandle NbodyHandle;

enum {
    NBODY_OK = 0,
    NBODY_ERR_INVALID = -1,     /* bad argument / call not valid in this state */
    NBODY_ERR_HIP = -2,         /* a HIP runtime call failed */
    NBODY_ERR_CAPACITY = -3,    /* more bodies than the handle was created for */
    NBODY_ERR_TREE_DEPTH = -4,  /* octree deeper than NBODY_MAX_TREE_DEPTH (coincident bodies): the
                                   reference recurses without bound here (barnes_hut.rs:143-183) */
    NBODY_ERR_COMM = -5,        /* RCCL failure */
    NBODY_ERR_NO_DEVICE = -6    /* no usable HIP device */
};

#define NBODY_MAX_TREE_DEPTH 192

/* which reference solver the handle stands in for */
enum { NBODY_BRUTE_FORCE = 0,  /* src/manual/brute_force.rs */
       NBODY_BARNES_HUT = 1 }; /* src/manual/barnes_hut.rs  */

/* arithmetic of the force kernels */
enum { NBODY_MATH_STRICT = 0, /* sqrt, (d*d)*d, g/r^3, no FMA contraction, partners in ascending
                                 index order: the reference's rounding sequence */
       NBODY_MATH_FAST = 1 }; /* v_rsq_f32, FMA, partner range split over waves: <=1e-5 relative */

/* where the Barnes-Hut octree is built */
enum { NBODY_TREE_HOST = 0,    /* host, every step (north_star; barnes_hut.rs:143-183 bit for bit) */
       NBODY_TREE_DEVICE = 1,  /* device: same cells and links, centre-of-mass
                                  sums in a different order (double-double prefix sums), so node counts may differ
                                  by a few parts in 1e4; <= 42 levels (a deeper step is built on the host).
                                  Single-shard handles enqueue their steps without any read-back */
       NBODY_TREE_AUTO = 2 };  /* NBODY_MATH_FAST -> device, NBODY_MATH_STRICT -> host (the bit-exact path);
                                  what the host-side mirrors pass by default */

/* Barnes-Hut leaf semantics */
enum {
    NBODY_LEAF_REFERENCE = 0, /* src/manual/barnes_hut.rs:185-203: a leaf failing the opening test contributes 0 */
    NBODY_LEAF_DIRECT = 1     /* the walk of src/llm/barnes_hut.rs:915-997 on the same tree: a node closer than
                                 r2 < 1e-10 is skipped whole (how a body skips itself), a leaf failing the opening
                                 test is evaluated directly; force = d * (g*mass * (1/sqrt(r2+eps2))^3) */
};

/* the reference's `F: Float` (src/shared.rs:12-44) */
enum { NBODY_F32 = 0,  /* PointParticle<f32,3>: every path of this library */
       NBODY_F64 = 1 }; /* PointParticle<f64,3> (80-byte records).  Brute force: NBODY_MATH_STRICT the reference's loop (bit-exact),
                          NBODY_MATH_FAST every unordered pair once (rsqrt + FMA, planes added in a fixed order: each body
                          within 1e-14 of the sum of its terms' magnitudes).  Barnes-Hut, NBODY_MATH_STRICT: the
                          reference's nested sums on the host-built tree (NBODY_TREE_HOST, also what AUTO means then): positions,
                          velocities, accelerations and node counts bit-equal to the reference's rounding sequence in f64 (oracle/:
                          the same templated restatement); with NBODY_TREE_DEVICE the tree is built on the device (same cells, centres
                          of mass to the last bits: node counts within 1e-6), ~4x the steps per second.  NBODY_MATH_FAST: one running
                          sum per lane (FMA, 1/sqrt) over a split node range, device build under AUTO: accelerations to 1e-12.
                          Worlds of several ranks: index-block shards (strict results bit-equal to one shard; the tree is built on the
                          host in strict math, by every rank on the device from the gathered positions in fast math) */

/* how the bodies are dealt to the shards of a multi-GPU run */
enum { NBODY_SHARD_INDEX = 0,   /* contiguous index blocks of the vector; positions all-gathered every step (every method) */
       NBODY_SHARD_SPATIAL = 1 }; /* Barnes-Hut, fast math, device build: ownership by Morton-key range (bodies that cross a
                                   boundary migrate), every rank builds only its slice of the tree and receives from each
                                   partner the nodes its own bodies can reach ("halo" / locally essential tree): configs[4] */

typedef struct NbodyConfig {
    uint32_t struct_size;  /* = sizeof(NbodyConfig) */
    int32_t method;        /* NBODY_BRUTE_FORCE | NBODY_BARNES_HUT */
    int32_t math_mode;     /* NBODY_MATH_STRICT | NBODY_MATH_FAST */
    int32_t leaf_mode;     /* NBODY_LEAF_REFERENCE (default) | NBODY_LEAF_DIRECT; Barnes-Hut only */
    int32_t device;        /* HIP device ordinal; -1 = LOCAL_RANK env or 0 */
    int32_t rank;          /* this process's shard, 0 <= rank < world_size */
    int32_t world_size;    /* number of shards (one process per GPU); 1 = single GPU */
    int32_t host_threads;  /* octree-build threads (the reference's `-t`, src/main.rs:34-35); 0 = all */
    uint64_t capacity;     /* max bodies over ALL shards (add_point may grow up to this) */
    int32_t tree_build;    /* NBODY_TREE_HOST | NBODY_TREE_DEVICE | NBODY_TREE_AUTO (Barnes-Hut only) */
    int32_t dtype;         /* NBODY_F32 (0, the default) | NBODY_F64 */
    int32_t shard_mode;    /* NBODY_SHARD_INDEX (0, the default) | NBODY_SHARD_SPATIAL; struct_size may also be the 48 bytes of */
    int32_t reserved;      /* ABI versions <= 2, which end before this field */
} NbodyConfig;

typedef struct NbodyStats {
    uint64_t steps;               /* step_by calls completed */
    uint64_t interactions;        /* bf: sum of n_own*(n_total-1) directed pairs; bh: accepted nodes */
    uint64_t node_visits;         /* bh: opening tests evaluated (0 for bf) */
    uint64_t tree_nodes;          /* bh: nodes in the last tree built */
    uint64_t force_launches;      /* dominant-kernel launches timed since the last nbody_reset_stats */
    uint64_t force_kernel_interactions; /* directed interactions those launches evaluated (bf: the
                                     symmetric kernel leaves ~2 % to a small companion kernel) */
    double force_kernel_ms;       /* sum of their HIP-event durations (needs nbody_set_profiling(h,1)) */
    double tree_build_ms;         /* bh: host wall time in the octree build, summed */
    double tree_copy_ms;          /* bh: host wall time in D2H positions + H2D nodes, summed */
    double exchange_ms;           /* multi-GPU: host wall time blocked in the exchange (0 when async) */
} NbodyStats;

/* ---- lifecycle: Simulation::new / Clone / drop ------------------------------------------- */
/* Simulation::new(points, integrator, bounds) (shared.rs:84): bodies and bounds arrive through
 * nbody_upload / nbody_set_bounds; the integrator is the reference's LeapFrogIntegrator
 * (shared.rs:106-149), the only one it ships.  Settings start at SimulationSettings::default()
 * (shared.rs:69-78): g=1, g_soft=0, dt=1e-3, theta2=0.5. */
int nbody_create(const NbodyConfig* cfg, NbodyHandle** out);
void nbody_destroy(NbodyHandle* h);
/* `Clone` supertrait (shared.rs:80; BH clone drops the tree, barnes_hut.rs:113-135; the visualiser's reset depends on it,
 * vis.rs:217-220).  Any handle; the clone of a sharded handle has no communicator: call nbody_comm_init on it. */
int nbody_clone(const NbodyHandle* h, NbodyHandle** out);
/* The configuration the handle runs with: tree_build after NBODY_TREE_AUTO and the spatial shards' override, math_mode as it
 * runs, the rest as created (struct_size = sizeof(NbodyConfig)). */
int nbody_get_config(const NbodyHandle* h, NbodyConfig* out);

/* ---- state in / out ------------------------------------------------------------------------ */
/* Replaces the body vector (the `points: Vec<P>` argument of Simulation::new).  In a sharded run
 * every rank passes the same full vector; the library keeps its own index block. */
int nbody_upload(NbodyHandle* h, const void* aos, size_t n, size_t stride_bytes);
/* Simulation::get_points (shared.rs:93).  Writes this rank's bodies (all of them when
 * world_size == 1) in vector order; *n_out = how many. */
int nbody_download(NbodyHandle* h, void* aos, size_t cap, size_t stride_bytes, size_t* n_out);
/* get_points().len() of this rank's block. */
int nbody_count(NbodyHandle* h, size_t* n_out);
/* Sum of nbody_count over all ranks as of the last exchange (== nbody_count when world_size == 1). */
int nbody_count_global(NbodyHandle* h, size_t* n_out);
/* Simulation::add_point = Vec::push (brute_force.rs:92-94).  In a sharded world a COLLECTIVE call (every rank passes the
 * same particle): the vector is the concatenation of the ranks' blocks, so the body goes to the end of the last rank's
 * block (NBODY_ERR_CAPACITY when that block is full); with NBODY_SHARD_SPATIAL to the rank that owns its key range, with
 * the next free index as its place in the vector. */
int nbody_add_point(NbodyHandle* h, const void* particle);
/* Simulation::remove_point = Vec::swap_remove (brute_force.rs:96-98): the world's last body takes the place of body `index`
 * (an index into the concatenated vector of all ranks; collective in a sharded world -- the body travels between ranks if
 * they differ).  NBODY_SHARD_SPATIAL: `index` counts the bodies in the order of their indices in the vector, as
 * nbody_download_ids reports them. */
int nbody_remove_point(NbodyHandle* h, size_t index);

/* ---- settings: Simulation::settings / settings_mut (shared.rs:95-96) ----------------------- */
int nbody_set_settings(NbodyHandle* h, float g, float g_soft, float dt, float theta2);
int nbody_get_settings(const NbodyHandle* h, float* g, float* g_soft, float* dt, float* theta2);
/* Bounds::new(center, width) (shared.rs:236-243). */
int nbody_set_bounds(NbodyHandle* h, const float center[3], float width);
/* The same for F = f64 (SimulationSettings<f64>, Bounds<f64, 3>).  Either set works on either kind of handle: the
 * f32 entry points widen exactly, the f64 ones round to f32 on an f32 handle. */
int nbody_set_settings_f64(NbodyHandle* h, double g, double g_soft, double dt, double theta2);
int nbody_get_settings_f64(const NbodyHandle* h, double* g, double* g_soft, double* dt, double* theta2);
int nbody_set_bounds_f64(NbodyHandle* h, const double center[3], double width);

/* ---- stepping ------------------------------------------------------------------------------- */
/* Simulation::init (brute_force.rs:47-50, barnes_hut.rs:229-236): elapsed = 0. */
int nbody_init(NbodyHandle* h);
/* Simulation::step_by(dt) (brute_force.rs:84-90, barnes_hut.rs:265-271): half drift, retain
 * in-bounds bodies, forces, kick + half drift, elapsed += dt.  dt may be negative. */
int nbody_step_by(NbodyHandle* h, float dt);
int nbody_step_by_f64(NbodyHandle* h, double dt);
/* k x Simulation::step() (shared.rs:86-88) with no host synchronisation in between (brute
 * force); returns after enqueueing.  Use nbody_sync before reading a host clock. */
int nbody_steps(NbodyHandle* h, int k);
/* Simulation::update_forces (brute_force.rs:64-82, barnes_hut.rs:250-263). */
int nbody_update_forces(NbodyHandle* h);
/* Simulation::elapsed (shared.rs:94). */
int nbody_elapsed(const NbodyHandle* h, float* out);
int nbody_elapsed_f64(const NbodyHandle* h, double* out);
/* Blocks until everything enqueued on the handle's stream has finished. */
int nbody_sync(NbodyHandle* h);

/* ---- diagnostics (no reference counterpart) -------------------------------------------------- */
int nbody_set_profiling(NbodyHandle* h, int on); /* HIP events around the force-kernel launches: 0 off, 1 every launch, k > 1 every k-th (an
                                                    event pair costs the stream ~11 us; the statistics then cover the bracketed launches) */
int nbody_stats(NbodyHandle* h, NbodyStats* out);
int nbody_reset_stats(NbodyHandle* h);
/* f64 kinetic and potential energy of this rank's view (world_size == 1: the whole system),
 * evaluated on the device: KE = sum 1/2 m v^2, PE = -g sum_{i<j} m_i m_j / sqrt(r^2 + g_soft^2). */
int nbody_energy(NbodyHandle* h, double* kinetic, double* potential);
/* Per-body potentials and the energy of a whole world (SURVEY.md section 8 row d), at the handle's CURRENT positions. */
enum { NBODY_POTENTIAL_PAIRS = 0,   /* the exact pair sum over every body of the world: differences, terms and sums in f64 on either
                                       dtype, every unordered pair of a block once; not for NBODY_SHARD_SPATIAL handles */
       NBODY_POTENTIAL_TREE  = 1,   /* Barnes-Hut handles: the monopole sum over the tree, O(N log N).  A tree is built first, as
                                       nbody_update_forces builds it for that handle (after the call nbody_tree_export reports THIS
                                       tree), and walked with the force walk's opening tests under the NBODY_LEAF_DIRECT rule
                                       whatever the handle's leaf_mode (a potential without its near field is of no use to anybody);
                                       terms m / sqrt(r2 + g_soft^2) in the handle's precision, summed in f64 */
       NBODY_POTENTIAL_TREE_QUADRUPOLE = 2 }; /* NBODY_POTENTIAL_TREE with the quadrupole term of every accepted INTERNAL cell: see
                                       "quadrupole terms in the tree potentials" below */
/* phi_i = -g * sum_j m_j / sqrt(|x_j - x_i|^2 + g_soft^2) for this rank's bodies, in nbody_download's order, in f64 on
 * either dtype.  Collective on a handle of a multi-rank world.  counts (may be NULL) = {terms summed, opening tests} of
 * this call on this rank (PAIRS: 0, 0).  phi may be NULL to count.  Accelerations, velocities, positions, elapsed and
 * NbodyStats.steps / interactions / node_visits are not touched: a step taken afterwards gives the bits it would have given
 * without the call.  NBODY_SHARD_SPATIAL handles: TREE only (PAIRS: NBODY_ERR_INVALID, a rank does not hold the world's bodies); no
 * body migrates and no ownership bound moves because of the call -- the pass runs on a scratch copy of the rank. */
int nbody_potentials(NbodyHandle* h, int mode, double* phi, size_t cap, size_t* n_out, uint64_t counts[2]);
/* KE = sum 1/2 m v^2 and PE = 1/2 sum_i m_i phi_i over ALL ranks (the same two numbers on every rank); collective. */
int nbody_energy_world(NbodyHandle* h, int mode, double* kinetic, double* potential);
/* The field of the world's bodies at caller-chosen points, at the handle's CURRENT positions:
 *   acc(x) = g * sum_j m_j (x_j - x) / (|x_j - x|^2 + g_soft^2)^(3/2),   phi(x) = -g * sum_j m_j / sqrt(|x_j - x|^2 + g_soft^2)
 * over ALL bodies of the world.  xyz: n_points f64 triples on either dtype; an f32 handle rounds each coordinate to the nearest
 * f32 once and the result is the field at the rounded point (a probe at a body's stored position coincides with it).  acc
 * [n_points][3] and phi [n_points] are f64, in the caller's order; either may be NULL, both NULL only counts.  n_points == 0 is
 * valid (TREE still builds its tree).  counts (may be NULL) = {terms summed, opening tests} of this call (PAIRS: 0, 0).
 *   NBODY_POTENTIAL_PAIRS  either method: coordinates widened to f64, differences, terms and sums in f64; a body at r2 == 0
 *                          exactly is skipped.
 *   NBODY_POTENTIAL_TREE   Barnes-Hut handles with bounds set: the tree nbody_update_forces would build (nbody_tree_export
 *                          reports it afterwards), walked with nbody_potentials(TREE)'s tests -- r2 in the handle's precision, a
 *                          node with r2 < 1e-10 skipped whole, w2 < theta2 * r2 accepts, a leaf that fails is evaluated whatever
 *                          the handle's leaf_mode.  Terms in the handle's precision (q = r2 + g_soft^2, inv = 1 / sqrt(q), scalar
 *                          m * inv, vector d * ((m * inv) / q)), the four sums in f64.
 * math_mode has no influence.  Points outside the box are legal; a point with a non-finite coordinate gets NaN outputs and
 * disturbs no other point.  TREE works in the handle's number range: a finite point so far away that r2 overflows (beyond
 * ~1e19 from the bodies on an f32 handle) gets exact zeros.  The same call twice gives the same bits, and permuting the points permutes the results bit for bit.
 * Collective on a world of index-block shards: every rank passes its own points (possibly none) and gets the whole world's field
 * at them.  NBODY_SHARD_SPATIAL handles are refused (NBODY_ERR_INVALID): a rank holds neither the world's bodies nor the tree
 * around a foreign point.  Like nbody_potentials the call leaves no trace in the state, the statistics or a later step. */
int nbody_field_at(NbodyHandle* h, int mode, const double* xyz, size_t n_points, double* acc, double* phi, uint64_t counts[2]);
/* The tidal tensor of the world's bodies at caller-chosen points, the gradient of nbody_field_at's acceleration, at the handle's
 * CURRENT positions:
 *   T_ab(x) = d acc_a / d x_b = g * sum_j m_j [ 3 d_a d_b / q^(5/2) - delta_ab / q^(3/2) ],   d = x_j - x,  q = |d|^2 + g_soft^2
 * over ALL bodies of the world (symmetric; trace -3 g g_soft^2 sum m / q^(5/2), zero without softening).  Self-gravity only:
 * the external field is not included.  xyz: n_points f64 triples on either dtype; an f32 handle rounds each coordinate to the
 * nearest f32 once.  tidal6 [n_points][6] f64 = {xx, xy, xz, yy, yz, zz} (the order of nbody_tree_export_quadrupoles), in the
 * caller's order; NULL only counts.  n_points == 0 is valid (TREE still builds its tree); n_points > 2^30, or xyz == NULL with
 * points, is NBODY_ERR_INVALID.  counts as nbody_field_at: {terms summed, opening tests} of this call (PAIRS: 0, 0).
 *   NBODY_POTENTIAL_PAIRS  either method, either dtype: coordinates widened to f64, everything in f64; a body at r2 == 0
 *                          exactly is skipped, so a point on a body's stored position gets the tensor of the others.
 *   NBODY_POTENTIAL_TREE   Barnes-Hut handles with bounds set: nbody_field_at(TREE)'s tree (nbody_tree_export reports it
 *                          afterwards) and opening tests -- r2 in the handle's precision, a node with r2 < 1e-10 skipped whole,
 *                          w2 < theta2 * r2 accepts, a leaf that fails is evaluated whatever leaf_mode -- so counts equal
 *                          nbody_field_at(TREE)'s for the same points.  Monopole terms in the handle's precision, six f64 sums.
 *   NBODY_POTENTIAL_TREE_QUADRUPOLE is refused (NBODY_ERR_INVALID): the quadrupole term's share of the tensor is out of scope.
 * A term, every line one rounding (IEEE sqrt and divide, no contraction): inv = 1 / sqrt(q), st = m inv, k = st / q,
 * k3 = (3 k) / q, u_c = d_c k3; xx += dx u_x - k (yy, zz alike), xy += dx u_y, xz += dx u_z, yz += dy u_z; each sum times g once.
 * math_mode has no influence.  A point with a non-finite coordinate gets six NaNs and disturbs no other point; under TREE a
 * finite point so far away that r2 overflows in the handle's precision gets exact zeros.  The same call twice gives the same
 * bits, and permuting the points permutes the rows bit for bit.  Accepted wherever nbody_field_at accepts the mode: collective
 * on a world of index-block shards (every rank passes its own points); NBODY_SHARD_SPATIAL handles are refused.  Like
 * nbody_field_at the call leaves no trace in the state, the statistics, the tracers or a later step. */
int nbody_tidal_at(NbodyHandle* h, int mode, const double* xyz, size_t n_points, double* tidal6, uint64_t counts[2]);
/* ---- quadrupole terms in the tree potentials: NBODY_POTENTIAL_TREE_QUADRUPOLE (no reference counterpart) --------
 * A mode of nbody_potentials, nbody_energy_world and nbody_field_at, chosen per call and independent of nbody_set_multipole
 * (which concerns the force pass only).  Everything that defines NBODY_POTENTIAL_TREE holds: the tree nbody_update_forces
 * would build (nbody_tree_export reports it afterwards), the NBODY_LEAF_DIRECT opening tests whatever the handle's leaf_mode
 * (r2 in f32 without contraction, r2 < 1e-10 skips the node whole, w2 < theta2 * r2 accepts, a leaf that fails is evaluated),
 * sums in f64, no trace in the state, the statistics or a later step, no influence of math_mode.  In addition an accepted
 * INTERNAL cell contributes its quadrupole term, Q being the tensor nbody_set_multipole describes below (about the stored f32
 * centre, f64 sums, 6 x f32): with d = c - x, q = |d|^2 + g_soft^2, inv = 1 / sqrt(q),
 *     S   += M inv + 1/2 (d^T Q d) inv^5                              (phi = -g S)
 *     acc += g [ M inv^3 d - inv^5 (Q d) + 2.5 inv^7 (d^T Q d) d ]    (= -grad phi: the force walk's term),
 * evaluated in f32 with IEEE sqrt and divide in u = d inv.  An accepted leaf contributes exactly NBODY_POTENTIAL_TREE's term,
 * so at theta2 = 0 the mode gives NBODY_POTENTIAL_TREE's bits, and counts equal NBODY_POTENTIAL_TREE's on any input.
 * nbody_field_at's contracts carry over: the same call twice gives the same bits, permuting the points permutes the results,
 * acc-only and phi-only calls give the combined call's bits, a non-finite point gets NaN and disturbs nobody, a finite point so
 * far away that r2 overflows gets exact zeros, n_points == 0 is valid.
 *   Accepted on Barnes-Hut, NBODY_F32, world_size == 1, NBODY_SHARD_INDEX handles with bounds set (either math mode, either
 * tree build, either leaf rule).  Brute-force handles, NBODY_F64 handles, handles of a multi-rank world and NBODY_SHARD_SPATIAL
 * handles get NBODY_ERR_INVALID: they are deliberately out of scope.  After a call in this mode nbody_tree_export_quadrupoles
 * reports the tensors the call used. */
/* Linearised octree of the last Barnes-Hut force pass: per node {com xyz, mass}, width, skip
 * index (first node after the subtree, depth-first pre-order).  Arrays may be NULL to count. */
int nbody_tree_export(NbodyHandle* h, float* com_mass, float* width, int32_t* skip, size_t cap, size_t* n_nodes);
int nbody_tree_export_f64(NbodyHandle* h, double* com_mass, double* width, int32_t* skip, size_t cap, size_t* n_nodes); /* f64 handles */
/* The cells of that octree for drawing: what the reference's Barnes-Hut Renderable walks (node.bounds.min() / .max() of
 * every node, barnes_hut.rs:322-343).  Per node, pre-order: {min xyz, max xyz} as f32 (the renderer casts to f32 anyway,
 * :331-333; an f64 handle's boxes are computed in double first) and its depth (root = 0).  Arrays may be NULL to count. */
int nbody_tree_export_cells(NbodyHandle* h, float* min_max6, int32_t* depth, size_t cap, size_t* n_nodes);
/* ---- order of the Barnes-Hut force walk's multipole expansion (no reference counterpart) ------------------------
 * NBODY_MULTIPOLE_MONOPOLE: an accepted cell acts as a point mass at its centre of mass (the reference's walk, and every
 * walk of this library by default).  NBODY_MULTIPOLE_QUADRUPOLE: an accepted INTERNAL cell also contributes its traceless
 * quadrupole tensor about its stored f32 centre of mass c,
 *     Q = sum_l m_l (3 d_l d_l^T - |d_l|^2 I),   d_l = c_l - c,   over the leaves l of the cell's subtree (a leaf: Q = 0),
 * computed on the device in f64 from the node array (either tree build) and kept as 6 x f32 per node beside the node
 * records.  With d = c - x, q = |d|^2 + g_soft^2, inv = 1 / sqrt(q) the term of an accepted internal cell is
 *     a += g [ M inv^3 d - inv^5 (Q d) + 2.5 inv^7 (d^T Q d) d ]      (the gradient of phi = -g [M inv + 1/2 d^T Q d inv^5]);
 * leaves contribute their monopole term as before, under the handle's leaf rule.  The opening tests do not change, so
 * NbodyStats.interactions and node_visits equal the monopole walk's on the same tree; the error per accepted cell falls by
 * one order in (cell width / distance).
 *   Accepted on Barnes-Hut, NBODY_F32, NBODY_MATH_FAST, world_size == 1 handles (either tree build, either leaf rule); every
 * other handle, and any order but 1 or 2, gets NBODY_ERR_INVALID.  NBODY_F64 handles and worlds of several ranks (index
 * blocks or NBODY_SHARD_SPATIAL) are deliberately out of scope: they walk monopoles.
 *   May be set at any time between calls; it takes effect at the next force pass (nbody_update_forces, nbody_step_by,
 * nbody_steps) and affects the force pass only: nbody_potentials(TREE) and nbody_field_at(TREE) stay monopole sums.  Setting
 * the order back to 1 restores the monopole path exactly (the same bits as a handle that never changed).  nbody_clone
 * carries the setting.  A handle with the device build keeps enqueueing its steps without read-back.  The walk runs one
 * body per lane over the node-range split: bh_walk_split, bh_walk_order and bh_reduce_split are honoured, bh_walk_duo is
 * ignored. */
enum { NBODY_MULTIPOLE_MONOPOLE = 1,     /* default */
       NBODY_MULTIPOLE_QUADRUPOLE = 2 };
int nbody_set_multipole(NbodyHandle* h, int order);
int nbody_get_multipole(const NbodyHandle* h, int* order);
/* The quadrupoles of the tree nbody_tree_export reports, in the same node order: 6 floats per node {xx, xy, xz, yy, yz, zz};
 * q6 may be NULL to count.  NBODY_ERR_INVALID unless the handle's last force pass walked with quadrupoles or its last tree
 * was built by a call in NBODY_POTENTIAL_TREE_QUADRUPOLE (a monopole force pass or an NBODY_POTENTIAL_TREE call after that
 * call: refused again). */
int nbody_tree_export_quadrupoles(NbodyHandle* h, float* q6, size_t cap, size_t* n_nodes);
/* ---- integrator: a fourth-order Hermite predictor-corrector beside the leapfrog (no reference counterpart) -------
 * The reference's Simulation is generic over an Integrator (shared.rs:99-104) and ships the leapfrog; this is the integrator of
 * direct-summation codes (Makino & Aarseth 1992).  It needs, per body, the jerk (the time derivative of the acceleration)
 * beside the acceleration.  With d = x_j - x_i, w = v_j - v_i, q = |d|^2 + g_soft^2, F(x, v) is the pair sum
 *     a_i = g sum_j m_j d / q^(3/2)          j_i = g sum_j m_j [ w - 3 (d.w)/q d ] / q^(3/2).
 * One step of size dt from (x0, v0) with the HELD derivatives (a0, j0):
 *     xp = x0 + v0 dt + a0 dt^2/2 + j0 dt^3/6           vp = v0 + a0 dt + j0 dt^2/2
 *     (a1, j1) = F(xp, vp)
 *     v1 = v0 + (a0 + a1) dt/2 + (j0 - j1) dt^2/12      x1 = x0 + (v0 + v1) dt/2 + (a0 - a1) dt^2/12
 * then retain (Bounds::contains' rule: inclusive walls, a NaN is outside; order preserved; bounds must be set) on the
 * CORRECTED positions, carrying pos, vel, acc and jerk together; (x1, v1, a1, j1) become the next (x0, v0, a0, j0), the acc
 * field of nbody_download is a1, elapsed += dt, NbodyStats.steps += 1, interactions += n (n - 1) per evaluation of F.  dt
 * may be negative.  Survivors of the retain keep their held (a0, j0): a departed body's pull leaves with the next
 * evaluation of F, one step later than its record.
 *   Accepted on NBODY_BRUTE_FORCE, NBODY_F64, world_size == 1 handles in either math mode.  Every other handle gets
 * NBODY_ERR_INVALID from nbody_set_integrator(NBODY_INTEGRATOR_HERMITE4), and so does any value but 0 or 1; NBODY_F32
 * handles, Barnes-Hut handles and worlds of several ranks are deliberately out of scope.  NBODY_INTEGRATOR_LEAPFROG is
 * valid on every handle.  A handle that never selects Hermite runs the leapfrog code untouched, and one that selects it and
 * the leapfrog again without a step in between gives the bits of one that never did.
 *   The held (a0, j0) are STALE after nbody_upload, nbody_add_point, nbody_remove_point, nbody_set_settings*, nbody_init
 * and a change of integrator: the next step (or nbody_suggest_dt) first evaluates F at the current (x, v), one more pass
 * that interactions counts.  nbody_update_forces on a Hermite handle evaluates F at the current state, stores a and j and
 * makes them valid.  nbody_clone carries the integrator, the jerk and the validity (and the handle's knobs): a clone
 * continues bit for bit like its source.  nbody_steps(k) enqueues k steps without a host synchronisation and gives the bits
 * of k nbody_step_by calls.
 *   NBODY_MATH_STRICT: one body per lane, partners j in ascending index order (j != i), IEEE sqrt and divide, every product
 * and sum rounded on its own (no FMA), in this order per pair and component c:
 *     d = x_j - x_i,  dv = v_j - v_i,  r2 = ((dx dx + dy dy) + dz dz) + g_soft^2,  rv = (dx dvx + dy dvy) + dz dvz,
 *     w = (g m_j) / (r2 sqrt(r2)),  al = (3 rv) / r2,  a_c += d_c w,  j_c += (dv_c - al d_c) w;
 * predictor and corrector, with dt2 = dt dt, c2 = dt2 0.5, c3 = (dt2 dt) / 6, h = dt 0.5, c12 = dt2 / 12 rounded once:
 *     xp = ((x0 + v0 dt) + a0 c2) + j0 c3,            vp = (v0 + a0 dt) + j0 c2,
 *     v1 = (v0 + (a0 + a1) h) + (j0 - j1) c12,        x1 = (x0 + (v0 + v1) h) + (a0 - a1) c12
 * (tests/hermite_ref.py restates all of it in numpy, bit for bit).  NBODY_MATH_FAST: every unordered pair once, rsqrt and
 * FMAs, partial sums added in a fixed order (the same input gives the same bits); predictor and corrector as above.  Each
 * body's acceleration within nbody_f64's fast brute-force bound, its jerk within 1e-12 of the sum of its terms' magnitudes.
 * The knobs bf64_min_bodies, bf64_rot and bf64_waves shape the fast pass as they do the leapfrog's; bf64_ipt: four bodies
 * per lane unless it is 8 (its default 0 means 4 here at every size). */
enum { NBODY_INTEGRATOR_LEAPFROG = 0, /* default: LeapFrogIntegrator (shared.rs:106-149) */
       NBODY_INTEGRATOR_HERMITE4 = 1 };
int nbody_set_integrator(NbodyHandle* h, int integrator);
int nbody_get_integrator(const NbodyHandle* h, int* integrator);
/* The held jerk j0 as [n][3] f64, in nbody_download's order; *n_out = how many.  NBODY_ERR_INVALID on a leapfrog handle and
 * while (a0, j0) are stale (jerk3 == NULL included). */
int nbody_download_jerk(NbodyHandle* h, double* jerk3, size_t cap, size_t* n_out);
/* eta * min_i |a_i| / |j_i| over the live bodies with |j_i| > 0 (+inf if there is none), norms sqrt((x^2 + y^2) + z^2) in
 * f64: reproducible from the downloaded arrays.  Evaluates F first if (a0, j0) are stale.  NBODY_ERR_INVALID on a leapfrog
 * handle and for eta <= 0. */
int nbody_suggest_dt(NbodyHandle* h, double eta, double* dt_out);
/* ---- block steps: individual time steps of a Hermite handle, quantised to powers of two (Makino & Aarseth 1992; no
 * reference counterpart) --------
 * nbody_set_block_steps(h, eta, max_level) with eta > 0 and 1 <= max_level <= 20 switches them on, (0, 0) off (the default).
 * They are a setting of a Hermite handle: accepted exactly where NBODY_INTEGRATOR_HERMITE4 is and only while it is selected
 * (a leapfrog handle, every handle that refuses HERMITE4 and every other (eta, max_level) get NBODY_ERR_INVALID, from all
 * five calls below); nbody_set_integrator(NBODY_INTEGRATOR_LEAPFROG) switches them off.  A handle that never switches them
 * on runs the shared-step code untouched, and one that switches them on and off again without a step in between gives the
 * bits of one that never did.
 *   One nbody_step_by(dt) is then a MACRO STEP.  With L = max_level it has T = 2^L ticks of tick = dt 2^-L (exact).  Body i
 * holds a level l_i in [0, L], a step of s_i = T >> l_i ticks, the tick tau_i of its last correction (all 0 at the start) and
 * (x0, v0, a0, j0) valid at tau_i.  Until every tau_i = T, one BLOCK STEP:
 *   1. tau* = min_i (tau_i + s_i); the ACTIVE SET is the bodies with tau_i + s_i == tau*, in ascending index order (integers).
 *   2. ALL bodies are predicted to tau*: dp_i = f64(tau* - tau_i) tick, c2 = (dp dp) 0.5, c3 = ((dp dp) dp) / 6,
 *      xp = ((x0 + v0 dp) + a0 c2) + j0 c3, vp = (v0 + a0 dp) + j0 c2.
 *   3. (a1, j1) = F(xp, vp) for the active bodies only; the partners are all n predicted bodies, the active ones included.
 *      NBODY_MATH_STRICT: the per-pair expressions above, partners j in ascending index order, j != i.  NBODY_MATH_FAST: rsqrt
 *      and FMAs, the partner range cut into slices whose sums are added in a fixed order (the same input gives the same
 *      bits); per row the bounds of the shared step's fast pass.
 *   4. the corrector on the active bodies with h_i = f64(s_i) tick in place of dt: h = h_i 0.5, c12 = (h_i h_i) / 12.
 *   5. the new level of each active body; per component c, every product and sum rounded on its own:
 *        da = a0 - a1,  h2 = h h,  h3 = h2 h,  a3_c = (da_c 12 + (j0_c + j1_c) (h 6)) / h3,
 *        a2_c = ((da_c (-6) - (j0_c 4 + j1_c 2) h) / h2) + a3_c h      (the second derivative at the END of the step),
 *        norms sqrt((x^2 + y^2) + z^2) of a1, j1, a2, a3,
 *        dtc = sqrt(eta ((|a| |a2| + |j| |j|) / (|j| |a3| + |a2| |a2|))),
 *        wanted level l*: l = 0; s = |dt|; while (s > dtc && l < L) { s *= 0.5; ++l; }   (a NaN dtc gives 0, dtc == 0 gives L);
 *      l* > l_i: l_i = l* (any finer step is commensurate); l* < l_i, l_i > 0 and tau* mod (T >> (l_i - 1)) == 0: l_i - 1 (a
 *      step doubles at most once, and only on its own grid); otherwise unchanged.
 *   6. tau_i = tau* for the active bodies; (x1, v1, a1, j1) become their held values.
 * Commensurability guarantees that the last block step ends with every body at T.  Then the retain on the corrected
 * positions, as the shared step does (no body leaves inside a macro step); the levels are carried with pos, vel, acc and
 * jerk.  elapsed += dt, NbodyStats.steps += 1, interactions += n_active (n - 1) per block step.  dt may be negative; the
 * levels depend on |dt| only.  dt == 0 takes the shared-step path.
 *   START LEVELS come from the held derivatives: dtc = eta (|a| / |j|), fed to the same loop.  They are assigned whenever
 * the levels are INVALID: wherever (a0, j0) are stale (above), after nbody_set_block_steps, after a shared step, and when
 * |dt| differs in bits from the previous macro step's.  nbody_update_forces on such a handle evaluates F and assigns start
 * levels for the settings' dt.  nbody_clone carries eta, max_level, the levels and their validity: the clone continues bit
 * for bit.  nbody_steps(k) gives the bits of k nbody_step_by calls; on a handle with block steps on it SYNCHRONISES WITH THE
 * HOST (once per block step: the schedule's 8 bytes are read back to size the force launch), everywhere else it stays
 * asynchronous.  tests/hermite_block_ref.py restates the macro step in numpy, bit for bit beside a strict handle. */
int nbody_set_block_steps(NbodyHandle* h, double eta, int max_level);
int nbody_get_block_steps(const NbodyHandle* h, double* eta, int* max_level);
/* The levels l_i, per body, in nbody_download's order; *n_out = how many.  NBODY_ERR_INVALID while the levels are invalid. */
int nbody_download_levels(NbodyHandle* h, int32_t* level, size_t cap, size_t* n_out);
/* out = {block steps, body updates (the sum of the active sets' sizes)} since nbody_reset_stats */
int nbody_block_step_counts(NbodyHandle* h, uint64_t out[2]);
/* test hook: F = (a, j) as [n_ids][3] f64 at the handle's CURRENT (x, v) for the listed bodies, through the active-set
 * kernels of the handle's math mode; ids distinct and < n, else NBODY_ERR_INVALID; leaves no trace in state or statistics */
int nbody_debug_hermite_forces_of(NbodyHandle* h, const int32_t* ids, size_t n_ids, double* acc3, double* jerk3);
/* ---- tracers: massless particles that ride in the bodies' field (no reference counterpart) ------------------------
 * A handle may hold, beside its bodies, a second vector of M TRACERS (PointParticle records; the mass field is ignored on
 * upload and written as 0 on download).  Tracers feel the bodies and exert nothing.  They are not bodies: they are in no tree,
 * they are not counted by nbody_count, nbody_download, nbody_energy*, nbody_potentials or nbody_field_at, they do not change
 * NbodyStats, and they never act on a body or on each other.  A handle that never uploads tracers runs the code it ran
 * before untouched, and one that uploads a tracer set and then an empty one without a step in between gives the bits of a
 * handle that never did.
 *   One nbody_step_by(dt) with tracers runs the reference's leapfrog (shared.rs:106-149) on BOTH vectors:
 *     1. half drift of bodies and tracers, x += (v * 0.5) * dt;
 *     2. retain of both by Bounds::contains (inclusive walls, a NaN is outside), order preserved, each vector on its own;
 *     3. the body force pass exactly as without tracers;
 *     4. the tracer force pass over the retained, half-drifted bodies;
 *     5. kick + half drift of both.
 * (The brute-force passes 3 and 4 read the same positions and write disjoint state; the library enqueues 4 first.  Under
 * Barnes-Hut 4 reads the tree of 3, not the bodies, and follows it.)
 * nbody_update_forces evaluates the tracers' accelerations too.  nbody_steps(k) gives the bits of k nbody_step_by calls and
 * stays enqueue-only: the live tracer count after a retain stays on the device, and launches are sized from the host's upper
 * bound, as for the bodies.  nbody_clone carries the tracers; nbody_upload of bodies leaves them alone.
 *   The tracer force pass, brute force:
 *     NBODY_MATH_STRICT  the strict body kernel's expression with no self index: a = 0, then for bodies j ascending
 *                        r = p_t - p_j, d = sqrt((rx rx + ry ry) + rz rz + g_soft^2), f = g / ((d d) d), a_c -= (r_c f) m_j;
 *                        no contraction, IEEE sqrt and divide.  These are the bits a zero-mass body appended after the
 *                        bodies gets from the reference's loop (brute_force.rs:64-82), as long as no two tracers coincide
 *                        (two coincident massless bodies give 0 * inf there when g_soft = 0; tracers never meet each other).
 *                        A tracer exactly on a body with g_soft = 0 gets NaN, as that appended body would.
 *     NBODY_MATH_FAST    the fast body kernel's pair arithmetic: d = p_j - p_t, an FMA chain into r2 = |d|^2 + g_soft^2,
 *                        v_rsq_f32, (m_j rinv) (rinv rinv), FMAs into three f32 sums, a = g * sum.  The body range is cut into
 *                        K slices (nbody_host_tracer_plan) whose partial sums are added in slice order.  No atomics: the same
 *                        input gives the same bits, and permuting the tracers permutes the results bit for bit.  Each
 *                        tracer is within (16 + n) 2^-24 g T of the exact sum, n = bodies, T = the sum of its terms'
 *                        magnitudes (tests/tracer_ref.py counts the roundings).
 *                        The plan is drawn from the tracer and body counts at their uploads, not from the live counts, so
 *                        the bits do not depend on when the caller reads a count back.
 *   The tracer force pass, Barnes-Hut (either math mode, either tree build): the tracers walk the tree the body force pass
 * has just built, before anything overwrites it.  They are visited in the Morton order of their positions and use the force
 * walk's opening tests (r2 = (x x + y y) + z z in f32 without contraction, w^2 < theta2 r2) and the handle's leaf rule: under
 * NBODY_LEAF_REFERENCE a leaf that fails the test adds nothing, under NBODY_LEAF_DIRECT a leaf is always added and a cell whose
 * centre of mass lies within 1e-5 of the tracer is skipped whole.  Every accepted node adds the fast walk's monopole term
 * (g m) rsq(r2 + g_soft^2)^3 (c - p) into three f32 sums; partial sums over runs of the walk's node-range segments are added in
 * run order, with no atomics.  The multipole setting does not apply: tracers walk MONOPOLES whatever nbody_set_multipole says,
 * and NBODY_MATH_STRICT handles use the same term.  There is no bit-exact claim here (zero-mass bodies would change the
 * reference's tree); a tracer is within 4.5e-6 T of the f64 sum of its own node list (tests/bh_list.py).  With the device
 * build the steps stay enqueue-only.
 *   Accepted on NBODY_F32, world_size == 1 handles of both methods.  NBODY_F64 handles and handles of a multi-rank world get
 * NBODY_ERR_INVALID from every tracer call: they are deliberately out of scope.  nbody_last_error names the call. */
/* Replaces the tracer set; n == 0 removes it.  capacity = the most tracers the handle may ever hold, 0 means n; n > capacity:
 * NBODY_ERR_CAPACITY. */
int nbody_tracers_upload(NbodyHandle* h, const void* aos, size_t n, size_t stride_bytes, size_t capacity);
/* Reads the live tracers back in vector order; the acc field holds the last tracer force pass, the mass field 0. */
int nbody_tracers_download(NbodyHandle* h, void* aos, size_t cap, size_t stride_bytes, size_t* n_out);
/* Number of live tracers. */
int nbody_tracers_count(NbodyHandle* h, size_t* n_out);
/* out = {directed interactions (live tracers x live bodies per pass; Barnes-Hut: accepted nodes), opening tests (0 under brute
 * force)} over the tracer force passes since nbody_reset_stats, counted on the device. */
int nbody_tracer_stats(NbodyHandle* h, uint64_t out[2]);
/* Host-only (no device needed), like nbody_host_launch_plan: the fast tracer pass's shape for n_tracers tracers and n_bodies
 * bodies; out = {tracers per lane, tracer groups (of 256 x tracers per lane), body slices K, slice length}.  Slice k covers
 * bodies [k * length, min(n_bodies, (k + 1) * length)). */
int nbody_host_tracer_plan(size_t n_tracers, size_t n_bodies, int out[4]);
/* ---- external field: static analytic potentials acting on bodies and tracers (no reference counterpart) -----------
 * A handle may hold up to NBODY_EXTERNAL_MAX COMPONENTS of a smooth background: a halo, a bulge, a disc, a central mass.  In
 * every kind d = x - center, and g is the handle's g as it stands at the pass.
 *   NBODY_EXT_PLUMMER         p = {M, b}, b >= 0 (b = 0: a point mass).  phi = -g M / sqrt(|d|^2 + b^2),
 *                             a = -g M d / (|d|^2 + b^2)^(3/2); the term is skipped (exact zeros) where |d|^2 + b^2 == 0.
 *   NBODY_EXT_HERNQUIST       p = {M, a}, a > 0, r = |d|.  phi = -g M / (r + a), acc = -g M d / (r (r + a)^2); the acceleration is
 *                             skipped where r == 0, phi is still evaluated there.
 *   NBODY_EXT_MIYAMOTO_NAGAI  p = {M, a, b}, a >= 0, b > 0, disc plane z = 0.  B = sqrt(dz^2 + b^2), D = dx^2 + dy^2 + (a + B)^2,
 *                             phi = -g M / sqrt(D), a_xy = -g M d_xy / D^(3/2), a_z = -g M dz (a + B) / (B D^(3/2)).
 *   NBODY_EXT_LOGARITHMIC     p = {v0, rc, qy, qz}, rc > 0, qy > 0, qz > 0; independent of g.
 *                             S = rc^2 + dx^2 + (dy/qy)^2 + (dz/qz)^2, phi = (1/2) v0^2 ln S, a = -v0^2 {dx, dy/qy^2, dz/qz^2} / S.
 * NBODY_ERR_INVALID (nbody_last_error names the call): a non-finite centre or parameter (all four p of every kind are
 * looked at: set the unused ones to 0), a parameter outside the ranges above, an unknown kind, a non-zero `reserved`,
 * n > NBODY_EXTERNAL_MAX.  On an NBODY_F32 handle the values must also be finite and in range once rounded to f32.
 *   THE ACCELERATION has one arithmetic, whatever math_mode says, in the handle's precision F: centre and parameters are
 * rounded to F once, sqrt and divide are IEEE, nothing is contracted, every product and sum is rounded on its own, in this
 * order (d_c = x_c - center_c first):
 *     PLUMMER         r2 = ((dx dx + dy dy) + dz dz) + b b;  r = sqrt(r2);  f = (g M) / (r2 r);  t_c = -(d_c f)
 *     HERNQUIST       r = sqrt((dx dx + dy dy) + dz dz);  ra = r + a;  f = (g M) / (r (ra ra));  t_c = -(d_c f)
 *     MIYAMOTO_NAGAI  B = sqrt(dz dz + b b);  aB = a + B;  D = (dx dx + dy dy) + aB aB;  f = (g M) / (D sqrt(D));
 *                     fz = (f aB) / B;  t_x = -(dx f),  t_y = -(dy f),  t_z = -(dz fz)
 *     LOGARITHMIC     yq = dy / qy;  zq = dz / qz;  S = ((rc rc + dx dx) + yq yq) + zq zq;  f = (v0 v0) / S;
 *                     t_x = -(dx f),  t_y = -((dy / (qy qy)) f),  t_z = -((dz / (qz qz)) f)
 * s = 0, then for the components in ascending order s_c += t_c (a skipped term adds exact zeros), and the pass's acceleration
 * becomes acc_c = acc_pass_c + s_c.  tests/external_ref.py restates this in numpy; the accelerations agree bit for bit in both
 * math modes.
 *   THE STEP with a field is the leapfrog as it stands -- half drift, retain, the force pass untouched, kick + half drift --
 * except that the acceleration the kick reads and nbody_download reports is acc_pass + s(x), x the half-drifted, retained
 * positions.  nbody_update_forces does the same without the kick.  Tracers get the same term at their own positions.
 * NbodyStats and nbody_tracer_stats do not change.  nbody_clone carries the field.  nbody_steps(k) gives the bits of k
 * nbody_step_by calls and stays enqueue-only wherever it is without a field.  A handle that never sets a field runs the code
 * it ran before untouched, and one that sets a field and removes it without a step in between gives the bits of one that
 * never did.
 *   THE POTENTIALS (nbody_external_potentials, nbody_external_energy, the phi of nbody_external_at) are f64 on either dtype:
 * positions widened, centre and parameters as given, the expressions above for phi (Plummer: 0 where skipped), summed over the
 * components in ascending order, at the handle's CURRENT positions.  nbody_external_at returns f64 acc from the acceleration
 * expressions in f64 -- the code of nbody_host_external_eval.  A probe with a non-finite coordinate gets NaN and disturbs no
 * other.  These calls leave no trace in state or statistics.
 *   nbody_energy*, nbody_potentials and nbody_field_at stay SELF-GRAVITY ONLY; the conserved total is
 * KE + PE + nbody_external_energy.
 *   Accepted on world_size == 1, NBODY_SHARD_INDEX handles running the leapfrog: both dtypes, both methods, both math modes,
 * every tree build and leaf rule, with or without tracers and nbody_set_multipole(2).  Deliberately out of scope, refused with
 * NBODY_ERR_INVALID: handles of a multi-rank world and NBODY_SHARD_SPATIAL handles (all five handle calls);
 * nbody_set_external_field with n > 0 while NBODY_INTEGRATOR_HERMITE4 is selected, and nbody_set_integrator(HERMITE4) while a
 * field is set (the Hermite step would need the field's jerk); time-dependent or moving components; the external term in
 * nbody_energy*, nbody_potentials or nbody_field_at. */
#define NBODY_EXTERNAL_MAX 8
enum { NBODY_EXT_PLUMMER = 0, NBODY_EXT_HERNQUIST = 1, NBODY_EXT_MIYAMOTO_NAGAI = 2, NBODY_EXT_LOGARITHMIC = 3 };
typedef struct NbodyExternalComponent {
    int32_t kind;
    int32_t reserved;
    double center[3];
    double p[4];
} NbodyExternalComponent;
/* Replaces the field; n == 0 removes it. */
int nbody_set_external_field(NbodyHandle* h, const NbodyExternalComponent* comps, size_t n);
/* The components as given; *n_out = how many even when `cap` are too few (NBODY_ERR_CAPACITY then). */
int nbody_get_external_field(const NbodyHandle* h, NbodyExternalComponent* comps, size_t cap, size_t* n_out);
/* phi_ext per body, in nbody_download's order; *n_out = how many. */
int nbody_external_potentials(NbodyHandle* h, double* phi, size_t cap, size_t* n_out);
/* sum_i m_i phi_ext(x_i): per block of 256 bodies a pairwise tree, the blocks in ascending order; no atomics, the same input
 * gives the same bits. */
int nbody_external_energy(NbodyHandle* h, double* potential);
/* The field of the handle at n_points probes (f64 triples): acc [n][3] and phi [n], either may be NULL. */
int nbody_external_at(NbodyHandle* h, const double* xyz, size_t n_points, double* acc, double* phi);
/* Host-only (no device needed), f64: the same for components and g given by the caller. */
int nbody_host_external_eval(const NbodyExternalComponent* comps, size_t n, double g, const double* xyz, size_t n_points,
                             double* acc, double* phi);
/* ---- diagnostics of the state as a whole: momentum, angular momentum, mass profile (no reference counterpart) -----
 * Two READ-ONLY calls on a handle's bodies, evaluated on the device, f64 on either dtype (positions, velocities and masses
 * widened; nothing contracted, every product, sum and difference rounded on its own).  "The bodies" are what nbody_download
 * would report at that moment -- on a Hermite handle the held (x0, v0).  Tracers are not bodies and are not counted; the
 * external field plays no part.  Both calls LEAVE NO TRACE: state, NbodyStats, tracers, the validity of a Hermite handle's
 * held derivatives, block-step levels and the bits of every later step are what they would be without the call (the contract
 * of nbody_potentials and nbody_external_energy).  They confirm steps enqueued without a read-back, but do not refresh the
 * host's view of the body count: the launches are sized from its upper bound and read the live count on the device, so the
 * result is right after a retain has dropped bodies, with no nbody_count in between.  Scratch is allocated and freed inside
 * the call.  No floating-point atomics: the same input gives the same bits.  Neither call has been timed on an MI355X; their
 * cost there is not measured.
 *   nbody_moments: out = {M, X[3], P[3], L[3]}, M = sum m, X = sum m x (the centre of mass is X / M: the caller divides),
 * P = sum m v, L = sum m (x cross v) about the origin.  Per body the terms are m, m x_c, m v_c and
 * l_x = (y vz - z vy) m, l_y = (z vx - x vz) m, l_z = (x vy - y vx) m.  Each of the ten sums has nbody_external_energy's
 * shape: per block of 256 bodies the pairwise tree sum[t] += sum[t + half] for half = 128 ... 1 (rows past the live count
 * hold +0.0), the block sums then added on the host in ascending block order, starting from +0.0.  tests/diag_ref.py restates
 * it in numpy, bit for bit.  No bodies: ten exact zeros.
 *   nbody_lagrangian_radii: radii[k] = the distance from `center` within which the fraction fractions[k] of the bodies' mass
 * lies.  center == NULL: the centre of mass X / M of nbody_moments, from the same arithmetic (M == 0 gives a NaN centre).
 * d = x - center, r2 = (dx dx + dy dy) + dz dz.  The bodies are ordered ascending by (r2, index in nbody_download's order); a
 * body whose r2 is NaN is left out of the order and of the mass, +inf is kept and comes last.  c_j = the inclusive prefix sum
 * of the masses in that order; *mass_out (may be NULL) = the last c_j; radii[k] = sqrt(r2) (IEEE) of the first body j with
 * c_j >= fractions[k] * mass_out, the product rounded once (found by binary search: negative masses, which make c_j fall,
 * are the caller's risk, and a target no prefix reaches gives NaN).  The prefix sums are this library's own double-double
 * scan with a fixed association order, rounded to f64 once at the end -- not rocPRIM's scan, whose grouping follows the
 * completion order of its tiles: every c_j lies within n 2^-53 sum|m| of the exact prefix (far closer in fact), and the same
 * call twice gives the same bits.  With no body left in the order every radius is NaN and *mass_out is 0.  n_frac == 0 is
 * valid.
 *   NBODY_ERR_INVALID (nbody_last_error names the call): out NULL; a fraction outside [0, 1] or NaN; n_frac > 2^20; fractions
 * or radii NULL with n_frac > 0.
 *   Accepted on every world_size == 1, NBODY_SHARD_INDEX handle: both dtypes, both methods, either math mode, any tree build,
 * leapfrog or Hermite, block steps on or off, with or without tracers, an external field or nbody_set_multipole(2).
 * Deliberately out of scope, refused with NBODY_ERR_INVALID: handles of a multi-rank world and NBODY_SHARD_SPATIAL handles. */
int nbody_moments(NbodyHandle* h, double out[10]);
int nbody_lagrangian_radii(NbodyHandle* h, const double center[3], const double* fractions, size_t n_frac, double* radii,
                           double* mass_out);
/* ---- binary census: every body's closest partner in two-body energy, and the mutual bound pairs (no reference counterpart)
 * Two READ-ONLY calls under the contract of the diagnostics above: "the bodies" are what nbody_download would report (on a
 * Hermite handle the held (x0, v0)), tracers and the external field play no part, the calls LEAVE NO TRACE in state,
 * NbodyStats, the validity of a Hermite handle's held derivatives, block-step levels or the bits of any later step, they do
 * not refresh the host's view of the body count (launches sized from its upper bound, the live count read on the device:
 * right after a retain with no nbody_count in between), scratch is allocated and freed inside the call, and there are no
 * floating-point atomics: the same state gives the same bits.
 *   THE PAIR ENERGY is f64 on either dtype: an NBODY_F32 handle's positions, velocities, masses, g and g_soft are widened
 * exactly.  Every product, sum and difference is rounded on its own, sqrt and divide are IEEE, nothing is contracted:
 *     d = x_j - x_i,  w = v_j - v_i,  soft2 = g_soft g_soft
 *     r2 = ((dx dx + dy dy) + dz dz) + soft2
 *     w2 = (wx wx + wy wy) + wz wz
 *     e_ij = 0.5 w2 - (g (m_i + m_j)) / sqrt(r2)
 * e_ij == e_ji BIT FOR BIT: negation is exact, so d and w have the same squares either way, and the sum of the two masses
 * commutes.  tests/pairs_ref.py restates both calls in numpy; the device's results are its bits.
 *   nbody_partners: partner[i] = the j != i with the smallest e_ij, among equal energies the lowest j; energy[i] = that
 * minimum.  A NaN energy never wins.  A body with no partner -- n == 1, or every e_ij NaN or +inf -- gets partner -1 and
 * energy +inf.  Coincident bodies without softening give e = -inf by IEEE rules, which DOES win.  Indices are those of
 * nbody_download's order.  Either array may be NULL; with both NULL the call only counts.  *n_out (may be NULL) = the bodies;
 * cap < n returns NBODY_ERR_CAPACITY with *n_out set and the arrays untouched.
 *   nbody_bound_pairs: the MUTUAL pairs -- partner[i] == j, partner[j] == i, e_ij < 0 -- once each with i < j, in ascending i.
 * The elements are computed on the device in the arithmetic written beside the fields below, with M = m_i + m_j, gm = g M,
 * e = e_ij (softened as above; the separation is not), h = d cross w formed as hx = dy wz - dz wy, hy = dz wx - dx wz,
 * hz = dx wy - dy wx, and h2 = (hx hx + hy hy) + hz hz.  A pair at e = -inf is listed (semi_major 0, period 0).  The list is
 * compacted on the device with an integer prefix sum (rocPRIM's scan: integer addition is associative, its order cannot
 * show); only the *n_pairs records cross to the host.  *binding_sum (may be NULL) = the sum of `binding` over the list in list
 * order, starting from +0.0.  pairs == NULL only counts (and still sums, if asked); cap < n_pairs returns NBODY_ERR_CAPACITY
 * with *n_pairs set, pairs and *binding_sum (0) carrying nothing.  n_pairs may be NULL.
 *   COST: O(N^2) f64 pair terms, each with an IEEE sqrt and an IEEE divide -- one body per lane, partners staged through LDS,
 * the grid (groups of 256 bodies) x K partner slices sized by the bf64_waves knob, the K records of a body merged in slice
 * order, so the result does not depend on K.  It has NOT been measured on an MI355X beyond the single run of
 * tools/pairs_bench.py that DESIGN 3.16 records (about 0.12 s at 262 144 bodies); nothing asserts or promises a time.
 *   Accepted on every world_size == 1, NBODY_SHARD_INDEX handle: both dtypes, both methods, either math mode, leapfrog or
 * Hermite, block steps on or off.  Refused with NBODY_ERR_INVALID (nbody_last_error names the call): handles of a multi-rank
 * world and NBODY_SHARD_SPATIAL handles. */
typedef struct NbodyBoundPair {
    int32_t i, j;          /* indices in nbody_download's order, i < j */
    double energy;         /* e_ij above, < 0 */
    double binding;        /* ((m_i m_j) / M) e, M = m_i + m_j */
    double semi_major;     /* gm / (-2.0 e), gm = g M */
    double eccentricity;   /* sqrt(q > 0 ? q : 0), q = 1 + ((2 e) h2) / (gm gm) */
    double period;         /* 6.283185307179586 * (a * sqrt(a / gm)) */
    double separation;     /* sqrt((dx dx + dy dy) + dz dz), unsoftened */
} NbodyBoundPair;
int nbody_partners(NbodyHandle* h, int32_t* partner, double* energy, size_t cap, size_t* n_out);
int nbody_bound_pairs(NbodyHandle* h, NbodyBoundPair* pairs, size_t cap, size_t* n_pairs, double* binding_sum);
/* ---- sticky mergers: every body's nearest body, the mutual contacts within a radius, and their merger (no reference
 * counterpart) -----
 * The "sticky sphere" rule of direct N-body codes: two bodies closer than a merge distance become one body at their centre of
 * mass, with their total mass and momentum.  nbody_nearest and nbody_contacts are READ-ONLY calls under the exact contract of
 * the binary census above (the bodies are what nbody_download would report, no trace in state, NbodyStats, validity flags or
 * the bits of any later step, no refresh of the host's view of the count, launches sized from its upper bound: right after a
 * retain with no nbody_count in between, scratch inside the call, no floating-point atomics).  nbody_merge_contacts WRITES.
 *   THE METRIC is f64 on either dtype (an NBODY_F32 handle's positions are widened exactly), unsoftened, nothing contracted:
 *     d = x_j - x_i,  r2 = (dx dx + dy dy) + dz dz
 * r2_ij == r2_ji BIT FOR BIT.  tests/merge_ref.py restates all three calls in numpy; the device's results are its bits.
 *   nbody_nearest: nearest[i] = the j != i of least r2, among equal r2 the lowest j; dist2[i] = that r2.  A NaN r2 never wins.
 * A body with no partner -- n == 1, or every r2 NaN -- gets -1 and +inf.  r2 == +inf cannot win either: a candidate replaces
 * the best so far on r2 < best only, which is false against the initial +inf, so a body whose every r2 is +inf or NaN also
 * gets -1 and +inf.  Either array may be NULL; with both NULL the call only counts.  *n_out (may be NULL) = the bodies;
 * cap < n returns NBODY_ERR_CAPACITY with *n_out set and the arrays untouched.
 *   nbody_contacts: the MUTUAL pairs -- nearest[i] == j, nearest[j] == i -- with r2 < R2, R2 = radius * radius rounded once,
 * the comparison STRICT; once each with i < j, in ascending i.  w = v_j - v_i, w2 = (wx wx + wy wy) + wz wz, in f64 from the
 * widened values; `into` is filled as if the merge happened.  list == NULL only counts; cap < n_contacts returns
 * NBODY_ERR_CAPACITY with *n_contacts set and the list carrying nothing.  n_contacts may be NULL.
 *   nbody_merge_contacts: the same list, then applied.  list != NULL with cap < n_contacts returns NBODY_ERR_CAPACITY with
 * *n_contacts set and the state UNTOUCHED (the check comes before any write); list == NULL merges and reports the count.  For
 * each pair, in f64, every operation rounded on its own:
 *     M = m_i + m_j
 *     q_c = ((m_i q_i,c) + (m_j q_j,c)) / M      q in {position, velocity, acceleration}, per component c
 * (M == 0: q_c = (q_i,c + q_j,c) * 0.5); on a Hermite handle the held jerk is carried the same way; on an NBODY_F32 handle
 * each result and M are then rounded to f32 once.  The mass-weighted acceleration is the physically right one: the mutual
 * forces cancel.  The merged record replaces body i, body j is removed, and everybody else keeps their relative order --
 * Vec::retain's rule, carried out by the handle's own retain kernels.
 *   ONE CALL MERGES DISJOINT PAIRS ONLY; a clump of k bodies needs repeated calls, `while (n_contacts > 0)`.  That loop ends,
 * and ends with no pair left inside the radius: IF ANY PAIR HAS r2 < R2, AT LEAST ONE CONTACT IS FOUND.  At the global
 * minimum of r2 take the lowest index a that takes part in a minimal pair, and b = nearest[a]: r2_ab is minimal, and among
 * the bodies tied at that distance from b, a is the lowest index (every one of them takes part in a minimal pair), so
 * nearest[b] == a.  Each merging call removes at least one body.
 *   EFFECTS of a call that merged at least one pair are those of nbody_remove_point: the host's body count is exact
 * (n - n_contacts); a Barnes-Hut handle's tree and its exports are those of the state before the call until the next force
 * pass; a Hermite handle's held (a0, j0) are STALE and its block-step levels INVALID.  NbodyStats, tracers, the external
 * field, settings, bounds, elapsed, the integrator and the multipole order are untouched.  A call that found NO contact
 * leaves no trace at all, like the read-only calls.  Like nbody_remove_point the call first confirms enqueued steps.
 *   COST: O(N^2) f64 pair terms of 3 subtractions, 3 products, 2 sums and a compare -- nbody_partners' frame (one body per
 * lane, partners through LDS, groups x K slices sized by bf64_waves, the K records merged in slice order: the bits do not
 * depend on K) without velocities, sqrt or divide.  NOT MEASURED on an MI355X beyond the single run of tools/merge_bench.py that
 * DESIGN 3.17 records (about 0.03 s at 262 144 bodies); nothing asserts or promises a time.
 *   Accepted on every world_size == 1, NBODY_SHARD_INDEX handle: both dtypes, both methods, either math mode, any tree build,
 * leapfrog or Hermite, block steps on or off, with or without tracers, an external field or quadrupoles.  Refused with
 * NBODY_ERR_INVALID (nbody_last_error names the call): radius not finite or <= 0 (the two calls that take one); handles of a
 * multi-rank world and NBODY_SHARD_SPATIAL handles (all three). */
typedef struct NbodyContact {
    int32_t i, j;        /* indices BEFORE the call, nbody_download's order, i < j: i survives, j is absorbed */
    int32_t into;        /* index of the merged body AFTER the merge: i minus the absorbed bodies below i */
    int32_t reserved;    /* 0 */
    double separation;   /* sqrt(r2), IEEE, unsoftened */
    double mass;         /* M = m_i + m_j */
    double dkinetic;     /* -0.5 (((m_i m_j) / M) w2) <= 0: kinetic energy the merger removes; 0 when M == 0 */
} NbodyContact;
int nbody_nearest(NbodyHandle* h, int32_t* nearest, double* dist2, size_t cap, size_t* n_out);
int nbody_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts);
int nbody_merge_contacts(NbodyHandle* h, double radius, NbodyContact* list, size_t cap, size_t* n_contacts);
/* ---- friends-of-friends groups: which bodies belong together, and the catalogue of the clumps (no reference counterpart) ---
 * The friends-of-friends (FoF) group finder of N-body work: two bodies closer than a linking length are friends, a group is a
 * connected component of the friendship graph.  Two READ-ONLY calls under the exact contract of the binary census and
 * nbody_nearest above (the bodies are what nbody_download would report -- on a Hermite handle the held (x0, v0) --, tracers
 * and the external field play no part, no trace in state, NbodyStats, validity flags, levels or the bits of any later step,
 * no refresh of the host's view of the count, launches sized from its upper bound and the live count read on the device:
 * right after a retain with no nbody_count in between, scratch through the handle's registry and freed inside the call, no
 * floating-point atomics: the same state gives the same bits).
 *   THE LINK is nbody_nearest's metric, f64 on either dtype (an NBODY_F32 handle's positions are widened exactly), unsoftened,
 * nothing contracted:
 *     d = x_j - x_i,  r2 = (dx dx + dy dy) + dz dz
 * Bodies i and j are linked iff r2 < B2, B2 = linking_length * linking_length rounded once; the comparison is STRICT, as in
 * nbody_contacts.  A NaN r2 never links: a body with a NaN or infinite coordinate is A GROUP OF ITS OWN.  r2_ij == r2_ji bit
 * for bit, so the relation is symmetric and each unordered pair is looked at once.  tests/fof_ref.py restates both calls in
 * numpy; the device's results are its integers and its bits.
 *   nbody_fof_labels: label[i] = THE LOWEST INDEX in i's connected component (indices are those of nbody_download's order).
 * Pure integers, fully determined by the state: they do not depend on launch shape, scheduling or the bf64_waves knob.
 * *n_out (may be NULL) = the bodies; *n_groups_out (may be NULL) = the components among them, singletons included.
 * label == NULL only counts; cap < n returns NBODY_ERR_CAPACITY with *n_out and *n_groups_out set and the array untouched.
 *   nbody_fof_groups: the components with count >= min_members, in ascending `first`.  members holds their bodies, group after
 * group, each group in ascending index; offset and count index into it; *n_members is the total.  Either array may be NULL
 * (counts only); if either non-NULL array is too small the call returns NBODY_ERR_CAPACITY with both counts set and nothing
 * written.  n_groups and n_members may be NULL.  THE SEVEN SUMS of a group have a fixed association order.  With its members
 * k = 0 .. count-1 in ascending index:
 *     1. lane t = k mod 64 adds its terms in ascending k, starting from +0.0;
 *     2. the terms are m, m x_c and m v_c (f64 from the widened values), each product rounded once;
 *     3. then sum[t] += sum[t + half] for half = 32, 16, ... 1; the result is sum[0].
 * One wave per listed group does this; it mirrors the 256-wide tree of nbody_moments and nbody_external_energy.  The centre of
 * mass is mx / mass and the mean velocity mv / mass: the caller divides.
 *   HOW: an all-pairs pass on nbody_nearest's frame (one body per lane, partners through LDS, groups of 256 bodies x K slices
 * sized by bf64_waves, only j > i evaluated) whose lanes unite linked bodies in a lock-free union-find -- every write an
 * atomic compare-and-swap or minimum that lowers a word, nobody ever waits for anybody; afterwards the one root of a component
 * is its lowest index whatever the order of events was.  The catalogue is integer work: sizes by integer atomic adds, slots
 * and offsets by rocPRIM's integer scans, the member list by its stable radix sort.  Only the labels, or the listed records
 * and members, cross to the host.
 *   COST: O(N^2 / 2) f64 pair terms of 3 subtractions, 3 products, 2 sums and a compare, plus union-find traffic that depends
 * on the state (nothing for a world without links; a few atomic operations per linked pair).  NOT MEASURED on an MI355X beyond the
 * single run of tools/fof_bench.py that DESIGN 3.18 records (about 0.025 s at 262 144 bodies of a Plummer sphere with few
 * links, against 0.030 s of nbody_nearest); nothing asserts or promises a time.
 *   Accepted on every world_size == 1, NBODY_SHARD_INDEX handle: both dtypes, both methods, either math mode, any tree build,
 * leapfrog or Hermite, block steps on or off, with or without tracers, an external field or quadrupoles.  Refused with
 * NBODY_ERR_INVALID (nbody_last_error names the call): a linking length that is not finite or is <= 0; min_members < 1;
 * handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without touching a device.
 *   OUT OF SCOPE: a tree-accelerated neighbour search; periodic boundaries; linking in velocity space; unbinding; group
 * finding on multi-rank or spatial handles; any change to an existing call. */
typedef struct NbodyGroup {          /* 72 bytes */
    int32_t first;     /* lowest member index (nbody_download's order) = the group's label */
    int32_t count;     /* members */
    int32_t offset;    /* of its members in the member list */
    int32_t reserved;  /* 0 */
    double mass;       /* sum m */
    double mx[3];      /* sum m x   (centre of mass = mx / mass: the caller divides) */
    double mv[3];      /* sum m v */
} NbodyGroup;
int nbody_fof_labels(NbodyHandle* h, double linking_length, int32_t* label, size_t cap, size_t* n_out, size_t* n_groups_out);
int nbody_fof_groups(NbodyHandle* h, double linking_length, int min_members, NbodyGroup* groups, size_t group_cap, size_t* n_groups,
                     int32_t* members, size_t member_cap, size_t* n_members);
/* ---- self-bound subsets of friends-of-friends groups: FoF, then iterative unbinding (no reference counterpart) ----------------
 * A FoF group says "these bodies are close"; it does not say "these bodies belong together": fly-through bodies, chance
 * alignments and bridges are in the catalogue too.  nbody_fof_bound_groups does what halo and cluster finders do next: it
 * evaluates every member's energy inside its own group, strips the unbound members, and repeats until nobody is unbound.
 * READ-ONLY under the exact contract of nbody_fof_groups above (the bodies are what nbody_download would report -- on a
 * Hermite handle the held (x0, v0) --, tracers and the external field play no part, no trace in state, NbodyStats, validity
 * flags, levels or the bits of any later step, no refresh of the host's view of the count, launches sized from its upper bound
 * and the live count read on the device: right after a retain with no nbody_count in between, scratch through the handle's
 * registry and freed inside the call, no floating-point atomics: the same state gives the same bits).
 *   STEP 0 is the FoF groups of nbody_fof_groups(linking_length, min_members): the same link, the same catalogue, and
 * nbody_set_pair_search is honoured; the nbody_pair_search_stats record is what that call would leave.  The unbinding passes
 * never use the grid.
 *   AN EVALUATION PASS.  For each listed FoF group take its members in ascending index at positions k = 0 .. fof_count-1.  The
 * group holds an alive flag per position, all 1 at the start.  Everything is f64 from exactly widened values, every product,
 * sum and difference is rounded on its own, sqrt and divide are IEEE, nothing is contracted.
 *     1. GROUP SUMS.  The seven sums (m, m x_c, m v_c) of the alive members in nbody_fof_groups' shape: lane t = k mod 64 adds
 *        its alive members in ascending k, starting from +0.0 -- k is the position in the FoF list, not a rank among the
 *        alive; a dead member adds nothing --, then sum[t] += sum[t + half] for half = 32 .. 1.  V_c = mv_c / mass.
 *     2. PER-MEMBER ENERGY.  For each alive i: soft2 = g_soft g_soft.  The partner list is cut into tiles of 256 consecutive
 *        positions (k div 256).  s = +0.0; for each tile in ascending order: p = +0.0; for k ascending in the tile, if k is
 *        alive and k != k_i:
 *            d = x_k - x_i,  r2 = ((dx dx + dy dy) + dz dz) + soft2,  p += m_k / sqrt(r2)
 *        then s += p -- every tile is added, also one with no live partner.  phi_i = -(g s);  u = v_i - V,
 *        u2 = (ux ux + uy uy) + uz uz,  e_i = 0.5 u2 + phi_i.  (The tile rule lets an implementation stage 256 partners through
 *        LDS; the result does not depend on any launch-shape knob.)
 *     3. VERDICT.  Member i is UNBOUND iff !(e_i < 0): a NaN energy is unbound, -inf is bound (coincident members without
 *        softening get -inf).
 *   THE LOOP of a group, passes t = 0, 1, ...: evaluate the alive set; if nobody is unbound stop with converged = 1; else if
 * t + 1 == max_iterations stop with converged = 0 -- nobody is removed by this last pass, so the reported energies always
 * describe the reported set --; else clear the alive flag of EVERY unbound member AT ONCE; if fewer than min_members remain
 * the group is DISSOLVED and is not listed.  iterations = t + 1.  Groups proceed independently.
 *   OUTPUT.  The surviving groups in ascending `first`; members holds their alive bodies, group after group, each in ascending
 * index; energy[k] (may be NULL) is the e_i of members[k] from the group's last pass.  kinetic and potential are sums in the
 * shape of step 1 over the alive members (k still the position in the FoF list) of the terms (0.5 m_i) u2_i and
 * (0.5 m_i) phi_i of the last pass; mass, mx and mv are the last pass's seven sums.  `first` stays the label of the FoF group
 * -- its lowest index, which need not be a bound member.  A converged group has every e_i < 0.  Compaction and offsets are
 * integer work (flags, rocPRIM integer scans, a stable order): the order of events cannot show.  tests/unbind_ref.py restates
 * the call in numpy; the device's results are its integers and its bits.
 *   NULL AND CAPACITY FORMS are nbody_fof_groups': any array may be NULL (the call only counts -- it still runs every pass);
 * a non-NULL array that is too small returns NBODY_ERR_CAPACITY with both counts set and nothing written.  energy is sized by
 * member_cap.  n_groups and n_members may be NULL.
 *   HOW: one launch chain per pass serves every group still running: one wave per group for the seven sums, then the energy
 * kernel -- one member per lane, a block per 256 consecutive positions of the FoF member list, so a group of n_g members is
 * spread over n_g / 256 blocks; where a block's rows share a group the tile of 256 partners is staged through LDS, where they
 * do not (small groups, the ends of a large one) each lane reads its own group's partners directly, in the same order --,
 * then one wave per group for the verdict.  The host reads back one integer per pass: the groups still running.
 *   COST: per pass, the sum over the groups still running of n_g^2 f64 pair terms (n_g = fof_count: dead positions are
 * skipped, not compacted), each with a sqrt and a divide, plus nbody_fof_groups' own cost once.  Scratch: nbody_fof_groups'
 * (48 bytes per body plus rocPRIM's temporaries) plus 48 bytes per listed FoF member and 184 bytes per listed FoF group (at
 * most 140 bytes per body in all at min_members = 2).  NOT MEASURED on an MI355X beyond the single run of
 * tools/fof_bound_bench.py that DESIGN 3.21 records (one run: about 0.073 s at 262 144 f64 bodies of a Plummer sphere plus six
 * blobs of 16 384, 13 passes and at least 7.5e9 pair terms, against 0.026 s of nbody_fof_groups on the same state); nothing
 * asserts or promises a time.
 *   Accepted wherever nbody_fof_groups is.  Refused with NBODY_ERR_INVALID (nbody_last_error names the call): everything
 * nbody_fof_groups refuses; min_members < 2; max_iterations < 1 or > 1024.  A NULL handle is refused without touching a
 * device.  Negative masses and g <= 0 are the caller's risk (with g <= 0 every group dissolves, which is correct).
 *   OUT OF SCOPE: stripping only the most unbound fraction per pass; tree-accelerated group potentials; substructure
 * (sub-halos, saddle points); a per-body bound-label array; unbinding of user-supplied member lists; periodic boundaries;
 * multi-rank and spatial handles; any change to an existing call. */
typedef struct NbodyBoundGroup {      /* 96 bytes */
    int32_t first;        /* label of the FoF group it came from (its lowest index), NOT necessarily a bound member */
    int32_t fof_count;    /* members of that FoF group */
    int32_t count;        /* bound members reported */
    int32_t offset;       /* of its bound members in the member list */
    int32_t iterations;   /* evaluation passes this group went through, >= 1 */
    int32_t converged;    /* 1: its last pass found nobody unbound; 0: stopped by max_iterations */
    double mass;          /* of the reported members */
    double mx[3];         /* sum m x */
    double mv[3];         /* sum m v */
    double kinetic;       /* sum (0.5 m_i) u2_i, u relative to the group's mean velocity */
    double potential;     /* sum (0.5 m_i) phi_i, phi from the reported members only */
} NbodyBoundGroup;
int nbody_fof_bound_groups(NbodyHandle* h, double linking_length, int min_members, int max_iterations,
                           NbodyBoundGroup* groups, size_t group_cap, size_t* n_groups,
                           int32_t* members, size_t member_cap, size_t* n_members,
                           double* energy /* [n_members], parallel to members; may be NULL */);
/* ---- neighbours within a radius: every body's neighbour list, local densities and the density centre (no reference
 * counterpart) -----
 * Who are all my neighbours within r, and how dense is it here?  Three READ-ONLY calls under the exact contract of nbody_nearest
 * and nbody_fof_labels above (the bodies are what nbody_download would report -- on a Hermite handle the held (x0, v0) --,
 * tracers and the external field play no part, no trace in state, NbodyStats, validity flags, levels or the bits of any later
 * step, no refresh of the host's view of the count, launches sized from its upper bound and the live count read on the device:
 * right after a retain with no nbody_count in between, scratch through the handle's registry and freed inside the call, no
 * floating-point atomics: the same state gives the same bits).  Fixed radius only: every body's k nearest neighbours are nbody_knn's, below.
 *   THE RELATION is nbody_nearest's metric and nbody_contacts' comparison, f64 on either dtype (an NBODY_F32 handle's positions
 * are widened exactly), unsoftened, nothing contracted:
 *     d = x_j - x_i,  r2 = (dx dx + dy dy) + dz dz,  R2 = radius * radius rounded once
 * j is a neighbour of i iff j != i and r2 < R2, STRICTLY.  NaN and +inf never qualify: a body with a non-finite coordinate
 * has no neighbours and is nobody's neighbour.  r2_ij == r2_ji bit for bit, so the relation is symmetric.
 * tests/within_ref.py restates all three calls in numpy; the device's results are its integers and its bits.
 *   nbody_neighbors_within: a CSR list.  The neighbours of body i are neighbor[offset[i] .. offset[i + 1]) in ASCENDING index
 * (indices are those of nbody_download's order); offset[0] = 0 and offset[n] = *n_neighbors_out, which is twice the number of
 * unordered pairs inside the radius.  Pure integers, fully determined by the state and the radius: they do not depend on
 * launch shape, scheduling, the bf64_waves knob or the search mode.  offset holds n + 1 entries and may be NULL; `cap` counts
 * bodies (an array of cap + 1 entries).  neighbor == NULL only counts; offset is still written if it is given.  *n_out (may
 * be NULL) = the bodies, *n_neighbors_out (may be NULL) = the directed neighbours.  If cap < n with offset non-NULL, or
 * neighbor_cap < *n_neighbors_out with neighbor non-NULL, the call returns NBODY_ERR_CAPACITY with both counts set and nothing
 * written.  A TOTAL ABOVE 2^31 - 1 DIRECTED NEIGHBOURS ALSO RETURNS NBODY_ERR_CAPACITY, with both counts set (the total is
 * counted in 64 bits) and a message that says to use a smaller radius: every device-side index and every rocPRIM size
 * argument stays inside 32 bits, and the library does not pretend otherwise.  nbody_density and nbody_density_center refuse
 * such a radius the same way.
 *   nbody_density: for each body the terms are its neighbours within `radius` AND THE BODY ITSELF, taken in ascending index; the
 * body's own term is evaluated at u = 0 without computing r2, so a body with a NaN coordinate gets its own term only.
 * count[i] = the number of terms (>= 1).  Masses are widened to f64, every product and sum is rounded on its own, sqrt and
 * divide are IEEE, and the sum s starts from +0.0 and runs in that one sequential order:
 *     NBODY_KERNEL_TOP_HAT       s += m_j;   rho = s / (4.1887902047863905 * ((radius radius) radius))
 *     NBODY_KERNEL_CUBIC_SPLINE  the M4 kernel of Monaghan & Lattanzio (1985) with support `radius`:
 *         hs = radius * 0.5,  u = sqrt(r2) / hs
 *         u < 1.0:    w = (1.0 - 1.5 (u u)) + 0.75 ((u u) u)
 *         otherwise:  t = 2.0 - u;  w = 0.25 ((t t) t)
 *         s += m_j w;   rho = s / (3.141592653589793 * ((hs hs) hs))
 * sqrt(fl(radius^2)) == radius in IEEE arithmetic and sqrt is monotonic, so sqrt(r2) <= radius for every neighbour, u <= 2
 * and t IS NEVER NEGATIVE: that is why there is no clamp.  Either output may be NULL; *n_out (may be NULL) = the bodies;
 * cap < n returns NBODY_ERR_CAPACITY with *n_out set and the arrays untouched.  The density is computed FROM THE CSR LIST of
 * nbody_neighbors_within, built in scratch by the same code -- that is what makes its bits independent of the search mode and
 * of the launch shape.  What it costs: scratch of 4 bytes per directed neighbour (8 under NBODY_SEARCH_CELLS, whose lists are
 * sorted out of place, plus rocPRIM's temporary storage) on top of 8 bytes per (body, partner slice).
 *   nbody_density_center: the density-weighted centre of Casertano & Hut (1985),
 *     center_c = (sum_i rho_i x_i,c) / (sum_i rho_i)       rho from nbody_density, each term rho_i x_i,c rounded once
 * The four sums have nbody_moments' shape: per block of 256 bodies the pairwise tree half = 128 ... 1, rows past the live
 * count adding +0.0, the block sums added on the host in ascending block order starting from +0.0; then three divides.
 * *rho_sum (may be NULL) = sum_i rho_i.  With no bodies the centre is NaN and *rho_sum is 0.  A body with a non-finite
 * coordinate has a finite density (its own term) and makes that coordinate of the centre non-finite, as it does for
 * nbody_moments.  The result is meant to be passed straight into nbody_lagrangian_radii(h, center, ...).
 *   HOW: under NBODY_SEARCH_ALL_PAIRS two passes on nbody_nearest's frame (one body per lane, partners through LDS, groups of
 * 256 bodies x K slices sized by bf64_waves) that both evaluate r2: a count pass writing the count of every (body, slice)
 * body-major, rocPRIM's integer exclusive scan over that array, and a fill pass writing each slice's neighbours in ascending j
 * at its place -- ascending lists without a sort, whatever K is.  Under NBODY_SEARCH_CELLS the same two passes walk the 27
 * cells around a body's own, and each list is then put into ascending order by rocPRIM's segmented radix sort of the integer
 * keys.  All of it is integer work: the order of events cannot show.  The densities are one lane per body walking its list.
 *   COST: all pairs: 2 N^2 f64 pair terms of 3 subtractions, 3 products, 2 sums and a compare; cells: O(N log N) for the grid
 * plus two pair terms per candidate pair and side, and the sort; either way one gather, and for the spline one sqrt and one
 * divide, per directed neighbour.  NOT MEASURED on an MI355X beyond the single run of tools/within_bench.py that DESIGN 3.20
 * records (262 144 bodies of a sparse Plummer world: about 0.057 s over all pairs against 0.030 s of nbody_nearest, about
 * 0.002 s over the cells); nothing asserts or promises a time.
 *   Accepted and refused exactly where nbody_fof_labels is: every world_size == 1, NBODY_SHARD_INDEX handle is accepted (both
 * dtypes, both methods, either math mode, any tree build, leapfrog or Hermite, block steps on or off, with or without tracers,
 * an external field or quadrupoles).  Refused with NBODY_ERR_INVALID (nbody_last_error names the call): a radius that is not
 * finite or is <= 0; an unknown kernel id; center NULL; handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL
 * handle is refused without touching a device.
 *   OUT OF SCOPE: k nearest neighbours (nbody_knn and nbody_knn_density, below); adaptive smoothing lengths; densities at arbitrary probe points; periodic boundaries;
 * multi-rank or spatial handles; any change to an existing call's results. */
enum { NBODY_KERNEL_TOP_HAT = 0,        /* the mass inside the sphere over its volume */
       NBODY_KERNEL_CUBIC_SPLINE = 1 }; /* the M4 spline with support `radius` */
int nbody_neighbors_within(NbodyHandle* h, double radius, uint64_t* offset /* [n + 1], may be NULL */, size_t cap,
                           int32_t* neighbor /* may be NULL: count only */, size_t neighbor_cap, size_t* n_out, uint64_t* n_neighbors_out);
int nbody_density(NbodyHandle* h, double radius, int kernel, double* rho, int32_t* count, size_t cap, size_t* n_out);
int nbody_density_center(NbodyHandle* h, double radius, int kernel, double center[3], double* rho_sum);
/* ---- k nearest neighbours: every body's exact k nearest bodies, and the Casertano-Hut density (no reference counterpart) -----
 * Who are my k nearest, however far they are?  Three READ-ONLY calls under the exact contract of nbody_nearest (the bodies are
 * what nbody_download would report -- on a Hermite handle the held (x0, v0) --, tracers and the external field play no part,
 * no trace in state, NbodyStats, validity flags, levels or the bits of any later step, no refresh of the host's view of the
 * count, launches sized from its upper bound and the live count read on the device: right after a retain with no nbody_count in
 * between, scratch through the handle's registry and freed inside the call, no floating-point atomics: the same state gives
 * the same bits).  The search is EXACT: no tree, no opening criterion, nothing approximated.
 *   THE METRIC is nbody_nearest's, formed as csrc/kernels_pairs.hip forms it, f64 on either dtype (an NBODY_F32 handle's
 * positions are widened exactly), unsoftened, nothing contracted into an FMA:
 *     d = x_j - x_i,  r2 = (dx dx + dy dy) + dz dz
 *   THE ORDER AND THE OUTPUTS: row i of neighbor and dist2 (k entries each, row-major [n][k], indices those of nbody_download's
 * order) holds the k bodies j != i that come first in the order (r2 ascending, then j ascending), in that order, and their r2.
 * A body enters only if r2 < +inf: a NaN or infinite r2 never enters, as in nbody_nearest.  A row with fewer than k such bodies
 * is padded with -1 and +inf.  nbody_knn(k = 1) is nbody_nearest, integer for integer and bit for bit.  tests/knn_ref.py
 * restates all three calls in numpy; the device's results are its integers and its bits.
 *   SIZES AND REFUSALS: cap and *n_out follow nbody_nearest's protocol; cap counts ROWS (arrays of cap k entries).  Either array
 * may be NULL; neighbor == NULL && dist2 == NULL only counts (*n_out = the bodies, nothing searched, stats zeroed).  cap < n
 * returns NBODY_ERR_CAPACITY with *n_out set and nothing written.  1 <= k <= NBODY_KNN_MAX_K, else NBODY_ERR_INVALID; k >= n is
 * valid and gives padded rows.  WHY 32: the bound keeps a block's 256 per-lane lists of (f64, i32) entries -- 256 x 32 x 12
 * bytes = 96 KiB -- within a CU's 160 KiB of LDS beside a partner tile of 8 KiB; the constant is part of the ABI wherever an
 * implementation keeps its lists.
 *   radius_hint AND THE PAIR SEARCH: THE RESULT NEVER DEPENDS on radius_hint, on the search mode, on the tuning knobs or on the
 * launch shape.  radius_hint must be 0 or finite and > 0, else NBODY_ERR_INVALID.  Under NBODY_SEARCH_ALL_PAIRS, or with
 * radius_hint == 0, or when the grid is not usable (pair search, below), every row is answered by the all-pairs pass.  Under
 * NBODY_SEARCH_CELLS with a hint the grid is drawn for length = radius_hint by the code of the fixed-radius calls; every
 * gridded row gathers its top k among the bodies of its 27 cells with r2 < R2 = radius_hint * radius_hint (rounded once).  A row
 * that found at least k is FINISHED: everything it did not see has r2 >= R2, which exceeds everything it kept, so
 * the answer is exact and no tie can straddle the boundary.  The rows that found fewer than k, and the rows that are not
 * gridded, are compacted in ascending index into a list, and a second all-pairs pass answers exactly the rows of that list.
 * There is no radius doubling and no iteration: a hint that is too small costs the all-pairs pass for the rows it failed, never
 * a wrong answer.  stats (may be NULL) = {rows answered from the cells, rows answered by the all-pairs pass}; their sum is *n_out.
 * nbody_pair_search_stats afterwards holds what a fixed-radius call with that length leaves when the cell search ran;
 * otherwise the record is unchanged.
 *   nbody_knn_density: Casertano & Hut's (1985) estimator, generalised to unequal masses.  k >= 2, else NBODY_ERR_INVALID.  For a
 * row whose list is complete (k neighbours), with masses widened to f64 and every operation rounded on its own:
 *     M = the masses of its first k - 1 neighbours, added sequentially in list order from +0.0
 *     r2 = dist2[k - 1],  r = sqrt(r2),  rho = M / (4.1887902047863905 * ((r r) r)),  rk2 = r2
 * (the constant and the association are NBODY_KERNEL_TOP_HAT's; the body itself and its k-th neighbour are not counted, as in
 * the paper).  A row whose list is incomplete gets rho = +0.0 and rk2 = +inf.  r == 0 -- k bodies coincident with the body --
 * gives the IEEE result of the division (+inf, or NaN for massless neighbours), reported as it is.  rho and rk2 [n] follow
 * nbody_density's protocol: either may be NULL, both NULL only counts, cap < n returns NBODY_ERR_CAPACITY with *n_out set.
 *   nbody_knn_density_center: nbody_density_center with that rho -- the same block sums (per block of 256 bodies the pairwise
 * tree), added on the host in ascending block order from +0.0, then three divides; *rho_sum (may be NULL) = sum_i rho_i.  With
 * no complete row the centre is NaN.  The result is meant to be passed straight into nbody_lagrangian_radii(h, center, ...).
 *   HOW: k_knn_pairs (csrc/kernels_knn.hip) on nbody_nearest's frame -- one row per lane, partners through LDS in tiles of 256,
 * groups of 256 rows x K slices sized by bf64_waves.  A lane keeps its sorted list in LDS as [slot][lane]; the r2 of the list's
 * last entry stands in a register as the admission threshold, so after the first tiles almost every partner costs one compare
 * beyond nbody_nearest's pair term.  k_knn_merge merges a row's K slice lists in ascending slice order under the same order, so
 * K cannot show.  k_cells_knn (csrc/kernels_cells.hip) walks the 27 cells with the same lists.
 *   COST: all pairs: N^2 f64 pair terms of 3 subtractions, 3 products, 2 sums and a compare, plus about k ln(N / k) insertions of
 * O(k) LDS moves per row.  Scratch: 12 k bytes per row for the result and as much per (row, slice).  NOT MEASURED on an MI355X
 * beyond the single run of tools/knn_bench.py that DESIGN 3.23 records; nothing asserts or promises a time.
 *   Accepted and refused exactly where nbody_neighbors_within is.  Refused with NBODY_ERR_INVALID (nbody_last_error names the
 * call): k or radius_hint as above; center NULL; handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle
 * is refused without touching a device.
 *   OUT OF SCOPE: k > 32; a tree search; approximate search; radius doubling or an iterated fallback; the neighbours of foreign
 * points; periodic boundaries; SPH gather / scatter kernels with per-body smoothing lengths (dist2[i k + k - 1] is what a
 * caller builds those from); multi-rank and spatial handles. */
enum { NBODY_KNN_MAX_K = 32 };
int nbody_knn(NbodyHandle* h, int k, double radius_hint, int32_t* neighbor /* [n][k] */, double* dist2 /* [n][k] */, size_t cap,
              size_t* n_out, uint64_t stats[2] /* may be NULL */);
int nbody_knn_density(NbodyHandle* h, int k, double radius_hint, double* rho /* [n] */, double* rk2 /* [n], may be NULL */, size_t cap,
                      size_t* n_out);
int nbody_knn_density_center(NbodyHandle* h, int k, double radius_hint, double center[3], double* rho_sum);
/* ---- pair-separation counts: how many pairs stand at each separation (no reference counterpart) -----
 * The calls above answer a question about one threshold.  These two count the pairs in every bin of separation at once --
 * DD(r), what the two-point correlation function, the radial distribution function and the correlation dimension are computed
 * from; the cross form (bodies against caller points) is the DR term of the Landy-Szalay estimator and, with one point, the
 * number profile in shells about a centre.  Two READ-ONLY calls under the exact contract of nbody_nearest and nbody_fof_labels
 * (the bodies are what nbody_download would report -- on a Hermite handle the held (x0, v0) --, tracers and the external field
 * play no part, no trace in state, NbodyStats, validity flags, levels or the bits of any later step, no refresh of the host's
 * view of the count beyond what nbody_neighbors_within does -- none --, launches sized from its upper bound and the live count
 * read on the device: right after a retain with no nbody_count in between, scratch through the handle's registry and freed
 * inside the call).  THE RESULT IS INTEGERS ONLY: it is exact, and it does not depend on launch shape, scheduling, the
 * bf64_waves, pair_hist_combine and pair_hist_flush knobs or the search mode.  No floating-point atomics anywhere.
 *   THE EDGES: n_bins + 1 of them, 1 <= n_bins <= NBODY_PAIR_COUNT_MAX_BINS.  E2[b] = edges[b] * edges[b], each rounded once in
 * f64.  Valid: every edge finite, edges[0] >= 0, every E2[b] finite and E2 STRICTLY ascending -- the squares, not the edges:
 * that is what rules out ties after rounding (1e-200 and 2e-200 both square to 0) and overflow (1e200).  Anything else, and
 * counts == NULL, is NBODY_ERR_INVALID and nbody_last_error names the call.
 *   THE METRIC is nbody_nearest's, formed as csrc/kernels_pairs.hip forms it, f64 on either dtype (an NBODY_F32 handle's
 * positions are widened exactly), unsoftened, nothing contracted into an FMA:
 *     d = x_j - x_i,  r2 = (dx dx + dy dy) + dz dz
 *   THE BIN RULE: the pair is counted in bin b iff E2[b] <= r2 && r2 < E2[b + 1] -- closed below, open above.  outside[0]
 * counts the pairs with r2 < E2[0]; outside[1] counts everything else, !(r2 < E2[n_bins]): a NaN or +inf separation (a body
 * with a non-finite coordinate) lands there and in no bin.  outside may be NULL.
 *   nbody_pair_counts covers every unordered pair i < j of live bodies, once.  INVARIANT:
 *     sum(counts) + outside[0] + outside[1] == n (n - 1) / 2       for the live count n, always.
 *   nbody_pair_counts_at covers every (body, point) pair, n m of them, with d = point - body, the same metric and the same
 * rule; a point that coincides with a body is a pair of r2 = 0 like any other (bin 0 when edges[0] == 0).  INVARIANT: the sum
 * is n m.  m == 0 is valid and gives all zeros; points == NULL with m > 0 is NBODY_ERR_INVALID; non-finite point coordinates
 * are allowed and land in outside[1].  points: m rows of {x, y, z} as doubles.
 *   Counts are 64 bits end to end: THERE IS NO CAPACITY REFUSAL (today's other route to DD(r), nbody_neighbors_within once per
 * edge, is refused as soon as a radius holds more than 2^31 - 1 directed neighbours).
 *   PAIR SEARCH: nbody_pair_counts reads nbody_set_pair_search (below).  Under NBODY_SEARCH_CELLS the grid is drawn for the
 * length |edges[n_bins]| and only the 27 surrounding cells are examined: every pair with r2 < E2[n_bins] is a candidate pair
 * there; outside[1] is then n (n - 1) / 2 less everything the walk counted, an integer subtraction -- bodies that cannot be
 * gridded are there by construction.  The record behind nbody_pair_search_stats is what the call leaves, with the candidates
 * counted as nbody_fof_labels counts them; a grid that cannot be drawn falls back to all pairs, as everywhere else.
 * nbody_pair_counts_at ALWAYS looks at all pairs and does not touch the record: a cell search for foreign points is out of
 * scope here.
 *   HOW: k_pair_hist (csrc/kernels_paircount.hip) on nbody_nearest's frame -- one body per lane, the partners (the bodies, or
 * the caller's points in batches of 2^20) through LDS in tiles of 256, groups of 256 bodies x K slices sized by bf64_waves;
 * in nbody_pair_counts a lane counts only j > i and whole tiles below a block's first row are skipped, so the work is N^2 / 2
 * pair terms.  E2 stands in LDS; the bin is a branch-free binary search over it, ceil(log2(n_bins)) steps, 10 for 1 024 bins.
 * Counts go to a block-private LDS histogram of 32-bit words with LDS integer atomics; the block adds its words to the call's
 * 64-bit array with vector integer atomics at its end -- and after every 65 535 tiles: 256 lanes x 256 partners x T tiles put
 * at most 65 536 T counts into one word, and 65 536 x 65 535 = 2^32 - 65 536 < 2^32 (the pair_hist_flush knob lowers T).  In a
 * clustered world most pairs fall into few bins and the lanes of a wave meet on one LDS word; the pair_hist_combine knob
 * selects the remedy: 0 none, 1 the lanes that share the first counting lane's slot add their number once (two ballots), 2
 * every distinct slot of the wave does.  Under NBODY_SEARCH_CELLS k_cells_pair_hist (csrc/kernels_cells.hip) walks
 * nbody_fof_labels' half of the 27 cells, every candidate pair once, with the same bin function and the same histogram; a
 * lane there sends its counts beyond the first 256 T straight to the 64-bit array, which keeps the same bound.
 *   COST: all pairs: N^2 / 2 (n m) f64 pair terms of 3 subtractions, 3 products and 2 sums, each followed by 2 + ceil(log2(n_bins))
 * LDS reads and compares and one LDS atomic.  NOT MEASURED on an MI355X beyond the single run of tools/pair_counts_bench.py
 * that DESIGN 3.22 records (f32 brute-force handles, log bins from 1e-3 to 32, whole calls): at 262 144 bodies of a Plummer
 * world about 0.184 s with 32 bins and 0.305 s with 1 024, 6.1 and 10.2 times nbody_nearest on the same handle (0.030 s, and
 * twice the pair terms); at 65 536 bodies 0.024 s and 0.040 s, 8.8 and 14.9 times.  A clumpy world with a third of its pairs
 * in one bin took the same time within 1.5 %: contention on the LDS words is not the limit, both combining forms of
 * pair_hist_combine were slower (1: by 10 to 14 %, 2: by a factor 1.8 to 4.8) and 0 is the default.  Over the cells with a
 * last edge of two mean spacings: 1.2 to 1.5 ms at 262 144 Plummer bodies, 12 to 20 ms in the clumpy world.  What limits the
 * all-pairs kernel has not been measured; nothing asserts or promises a time.
 *   Accepted and refused exactly where nbody_fof_labels is: every world_size == 1, NBODY_SHARD_INDEX handle is accepted (both
 * dtypes, both methods, either math mode, any tree build, leapfrog or Hermite, block steps on or off, with or without tracers,
 * an external field or quadrupoles).  Refused with NBODY_ERR_INVALID (nbody_last_error names the call): invalid edges or n_bins
 * as above; NULL counts; NULL points with m > 0; handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle
 * is refused without touching a device.
 *   OUT OF SCOPE: weighted (mass- or velocity-product) histograms -- they need a fixed-order float sum; periodic boundaries; a
 * cell search for nbody_pair_counts_at; multi-rank handles; the estimators built from the counts (xi, g(r)) -- README has the
 * two-line recipe. */
#define NBODY_PAIR_COUNT_MAX_BINS 1024
int nbody_pair_counts(NbodyHandle* h, const double* edges /* [n_bins + 1] */, int n_bins, uint64_t* counts /* [n_bins] */,
                      uint64_t outside[2] /* may be NULL */);
int nbody_pair_counts_at(NbodyHandle* h, const double* points /* [m][3] f64 */, size_t m, const double* edges, int n_bins,
                         uint64_t* counts, uint64_t outside[2] /* may be NULL */);
/* ---- grid deposit: the bodies assigned to a regular grid, NGP / CIC / TSC (no reference counterpart) ---------------------
 * Every call above answers a question at points.  nbody_deposit gives a field on a regular grid -- a column-density image, a
 * density cube, a momentum or m v^2 map, the input of a power spectrum or a particle-mesh step -- without nbody_download and
 * a host loop.  A READ-ONLY call under the contract of nbody_pair_counts (the bodies are what nbody_download would report --
 * on a Hermite handle the held (x0, v0) --, an NBODY_F32 handle's values are widened exactly, tracers and the external field
 * play no part, no trace in state, NbodyStats, tracers, validity flags, levels or the bits of any later step, no refresh of the
 * host's view of the count, launches sized from its upper bound and the live count read on the device: right after a retain
 * with no nbody_count in between, scratch through the handle's registry and freed inside the call).  The only thing a call
 * leaves behind is the record nbody_deposit_stats reads.
 *   THE SAME STATE GIVES THE SAME BITS, whatever the launch shape, the scheduling and the deposit_sort, deposit_combine and
 * deposit_lds knobs are: the cells accumulate in 64-bit FIXED POINT with integer additions, which are associative.  No
 * floating-point atomics anywhere.  A plain f64 scatter-add does not have this property: a 4 099-body Plummer world of unequal
 * masses deposited NGP on 16^3 cells differs in 109 cells between two orders of the bodies (tests/test_deposit_checker.py).
 *   THE ARITHMETIC (csrc/deposit_grid.h, restated in tests/deposit_ref.py), all f64, every operation rounded on its own,
 * nothing contracted into an FMA.  q is the body's quantity: m | m vx | m vy | m vz | m ((vx vx + vy vy) + vz vz) | 1.0.
 *     u_c = (x_c - origin_c) / spacing      on each axis c that is not ignored (project_axis)
 *     a body is SKIPPED when any of x, y, z, q is not finite, or when !(|u_c| < 2^31) on an axis that is not ignored
 *     NGP: i = floor(u), weight 1
 *     CIC: s = u - 0.5, i0 = floor(s), f = s - i0; cells i0, i0 + 1 get the weights 1.0 - f, f
 *     TSC: i = floor(u), d = (u - i) - 0.5, a = 0.5 - d, b = 0.5 + d; cells i - 1, i, i + 1 get 0.5 (a a), 0.75 - d d, 0.5 (b b)
 *     the ignored axis has one stencil cell, index 0, weight 1.0 (dims there must be 1): a column map
 *     a term is t = q ((wx wy) wz) into cell (ix, iy, iz)
 *     periodic: every index goes mod dims_c into [0, dims_c); otherwise a term whose cell is off the grid is dropped
 *   A body that is not skipped is INSIDE if every cell of its stencil lands on the grid (cells of weight zero included),
 * OUTSIDE if none does, PARTIAL otherwise; counts = {inside, partial, outside, skipped} add up to the live count n.  Under
 * periodic wrap partial and outside are 0.
 *   THE SCALE.  n = the live count (skipped bodies included), L = ceil(log2(n)) (0 for n = 1), e = the frexp exponent of the
 * largest |q| among the bodies that are not skipped (a maximum is exact in any order), S = 61 - e - L.  Every term becomes
 *     k = llrint(ldexp(t, S))    (ties to even);    acc[cell] += k  in int64;    grid[cell] = ldexp((double) acc[cell], -S)
 * No body, or every q zero: every cell is +0.0.  No cell can overflow: the weights of a body are non-negative and sum to
 * 1 (1 + eps), so sum |t| 2^S <= n 2^e 2^S (1 + eps) <= 2^61 (1 + eps), and rounding adds at most 27 n / 2 <= 2^35.
 *   WHAT IT COSTS IN ACCURACY: every term is rounded to 2^-(61 - L) of the heaviest body's q (2^-41 for 2^20 bodies), so a
 * cell is a DETERMINISTIC sum, not a correctly rounded one: its absolute error is at most (terms in the cell) / 2 of that
 * unit plus one final rounding, and a cell holding bodies 2^40 times lighter than the heaviest loses them.
 *   grid: [nx][ny][nz] row-major doubles, cap = the doubles it holds.  cap smaller than nx ny nz: NBODY_ERR_CAPACITY, grid
 * untouched.  grid == NULL: only counts is filled (cap is not looked at).  counts may be NULL.
 *   nbody_host_deposit is the same arithmetic on the host (no device needed) for n caller points {x, y, z} and their q; the
 * quantity field of the spec is ignored.  xyz or q NULL with n > 0, or n > 2^31 - 1, is NBODY_ERR_INVALID.
 *   nbody_deposit_stats: out = {1 once a call on this handle reached the device else 0, the plan of the last such call as
 * deposit_sort | deposit_combine << 1 | deposit_lds << 2, the terms that landed on the grid, the 64-bit atomics that went to
 * global memory}.  The last number depends on the plan and, with deposit_lds, on scheduling; nothing else does.  IT IS A
 * DIAGNOSTIC AID for tools/deposit_bench.py and the tests of the plans, NOT A STABLE CONTRACT: what the four words mean may
 * change with the kernels, and no program should decide anything by them.  The record is the one thing a call leaves behind.
 *   HOW (csrc/kernels_deposit.hip): k_deposit_q -- q of every row, the largest |q| by an integer atomicMax on its bits, the four
 * counts; k_deposit_keys and the stable rocPRIM radix sort that the cell search uses -- the rows ordered by home cell;
 * k_deposit -- one lane per body of that order: for every stencil offset the lanes of a wave whose terms hit the same cell
 * stand in a run, a segmented integer scan over the run by shuffles leaves the run's sum in its last lane, which alone adds
 * it -- to a block-private LDS table of 1 024 tagged int64 slots (deposit_lds = 1; a slot taken by another cell sends the
 * addition to global memory), or with one 64-bit vector atomic, relaxed, agent scope, to the cell; k_deposit_convert -- int64
 * to f64 in place; one copy to the host.  deposit_sort = 0, deposit_combine = 0, deposit_lds = 0 is the plain variant, one
 * atomic per term from unsorted bodies: the baseline and the cross-check.
 *   COST: O(N log N) for the sort, 1 | 8 | 27 terms per body, 8 bytes of scratch per cell and 24 per body beside the sort's
 * own.  NOT TIMED ON AN MI355X beyond the single run of tools/deposit_bench.py that DESIGN 3.24 records (2^20 Plummer bodies,
 * f32 handle, whole calls): 1.3 to 3.0 ms a call onto 128^3 and 512 x 512 x 1; the default plan (1, 1, 1) sends 5 to 15 times
 * fewer atomics to global memory than the plain variant, is 1.39 times faster for TSC on the cube and 2 to 13 % SLOWER in the
 * other five cases, where the call is mostly its fixed part; summed over the six cases three plans tie, the default among them.  The rate of 64-bit integer atomics itself, the kernels apart from the
 * call, f64 handles and denser worlds have not been measured.  Nothing asserts or promises a time.
 *   Accepted and refused on the handles of nbody_pair_counts.  Refused with NBODY_ERR_INVALID (nbody_last_error names the
 * call): spec NULL; an origin that is not finite; a spacing that is not finite or <= 0; a dimension < 1; nx ny nz >
 * NBODY_DEPOSIT_MAX_CELLS; an unknown scheme or quantity; project_axis outside -1 .. 2 or naming an axis whose dimension is
 * not 1; reserved != 0; handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without
 * touching a device.
 *   OUT OF SCOPE: anisotropic cells; higher-order (PCS) stencils; interlacing and the deconvolution of the window; per-axis
 * periodicity; the velocity moments' ratios (a dispersion map is three calls and a host division); multi-rank handles. */
#define NBODY_DEPOSIT_NGP 0
#define NBODY_DEPOSIT_CIC 1
#define NBODY_DEPOSIT_TSC 2
#define NBODY_DEPOSIT_MASS 0        /* q = m                                   */
#define NBODY_DEPOSIT_MOMENTUM_X 1  /* q = m vx                                */
#define NBODY_DEPOSIT_MOMENTUM_Y 2  /* q = m vy                                */
#define NBODY_DEPOSIT_MOMENTUM_Z 3  /* q = m vz                                */
#define NBODY_DEPOSIT_MV2 4         /* q = m ((vx vx + vy vy) + vz vz)         */
#define NBODY_DEPOSIT_NUMBER 5      /* q = 1.0                                 */
#define NBODY_DEPOSIT_MAX_CELLS 134217728   /* 2^27 */
typedef struct NbodyGridSpec {
    double origin[3];   /* the low corner of cell (0,0,0) */
    double spacing;     /* the cell's edge */
    int32_t dims[3];    /* nx, ny, nz >= 1, product <= NBODY_DEPOSIT_MAX_CELLS */
    int32_t scheme, quantity;
    int32_t periodic;   /* 0: terms that fall off the grid are dropped; 1: indices wrap on every axis */
    int32_t project_axis; /* -1, or 0/1/2: that axis is ignored (dims there must be 1): a column map */
    int32_t reserved;   /* 0 */
} NbodyGridSpec;
int nbody_deposit(NbodyHandle* h, const NbodyGridSpec* spec, double* grid /* [nx][ny][nz], row-major */, size_t cap,
                  uint64_t counts[4] /* inside, partial, outside, skipped; may be NULL */);
int nbody_host_deposit(const double* xyz /* [n][3] */, const double* q /* [n] */, size_t n, const NbodyGridSpec* spec,
                       double* grid, size_t cap, uint64_t counts[4]);
int nbody_deposit_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- grid sample: a grid read back at the bodies or at points, values and gradients (no reference counterpart) ------------
 * The transpose of nbody_deposit: the same NGP / CIC / TSC weights, the cells READ instead of added to.  With it a
 * particle-mesh step can be finished -- deposit the mass, solve Poisson's equation on the grid (nbody_grid_poisson below, or any FFT), sample the
 * potential's gradient at the bodies -- and a force found that way conserves momentum only when both directions use the same
 * assignment, which is why the call shares deposit_grid.h's stencil.  Also: the grid density at each body, a tabulated
 * background potential at tracer positions, a velocity field along a path.
 *   nbody_grid_sample samples at the handle's bodies: rows in nbody_download's order, *n_out = the live count, as nbody_knn
 * reports them; cap = the rows out (and cls) hold; cap smaller than the live count: NBODY_ERR_CAPACITY with *n_out set and
 * nothing written.  nbody_grid_sample_at samples at n_points caller points {x, y, z}: the handle lends its stream and its
 * memory only, as for nbody_external_at (it may hold no body).  Both are READ-ONLY calls under the contract of nbody_deposit;
 * the only thing a call leaves behind is the record nbody_grid_sample_stats reads.  nbody_host_grid_sample is the same
 * arithmetic on the host (no device needed).  The quantity field of the spec is ignored by all three.
 *   grid: [fields][nx][ny][nz] row-major doubles, fields in 1 .. NBODY_SAMPLE_MAX_FIELDS, fields nx ny nz <=
 * NBODY_DEPOSIT_MAX_CELLS.  out: [n][fields] (NBODY_SAMPLE_VALUE) or [n][3] (the gradients, which take one field).  cls
 * (may be NULL): each row's class; counts (may be NULL) = {inside, partial, outside, skipped}, which add up to n.
 *   THE ARITHMETIC (csrc/sample_grid.h, restated in tests/sample_ref.py), all f64, every operation rounded on its own, nothing
 * contracted into an FMA; an NBODY_F32 handle's positions are widened exactly first.  A gather has no addition-order problem:
 * THE SAME INPUT GIVES THE SAME BITS on the device, on the host and in the restatement, whatever the launch shape and the
 * sample_sort and sample_pregrad knobs are.
 *     the stencil of a point is the deposit's for q = 0.0: the skip rule, the weights, the ignored axis, the wrap
 *     VALUE, field f:   s = +0.0; for a, then b, then c innermost over the stencil's cells, a term whose cell is dropped
 *                       skipped:  w = (wx[a] wy[b]) wz[c];  s = s + w G_f[cell];  out[i][f] = s.  IEEE as it stands: a zero
 *                       weight times an infinite cell is NaN.
 *     GRADIENT, component k at stencil cell i:
 *         order 2:  D = (G[i + e_k] - G[i - e_k]) / (2.0 spacing)
 *         order 4:  D = (8.0 (G[i + e_k] - G[i - e_k]) - (G[i + 2 e_k] - G[i - 2 e_k])) / (12.0 spacing)
 *       the denominator is formed once per call; the neighbours' indices wrap when periodic (an axis of 1 or 2 cells then
 *       gives exact zeros); otherwise a term is dropped FOR THAT COMPONENT when a cell its difference reads is off the grid.
 *       out[i][k] = the sum of w D in VALUE's order; along project_axis it is +0.0 and nothing is read.  The result is +grad:
 *       the caller negates it for an acceleration.
 *     SKIPPED: the stencil refuses the point (a coordinate that is not finite, !(|u| < 2^31)); OUTSIDE: no stencil cell is on
 *     the grid; both give +0.0 everywhere.  INSIDE: every read of every component landed -- for a gradient that is the
 *     stencil widened by 1 or 2 cells on every axis in use; always when periodic.  PARTIAL: everything else.
 *   n == 0 (no body, no point): NBODY_OK, counts zeroed, nothing else written.
 *   nbody_grid_sample_stats: out = {1 once a call on this handle reached the device else 0, the plan the last such call USED as
 * sample_sort | sample_pregrad << 1, the grid reads k_sample issued, 0}.  A DIAGNOSTIC AID for tools/sample_bench.py and the
 * tests of the plans, NOT A STABLE CONTRACT.
 *   HOW (csrc/kernels_sample.hip): one copy of the grid to the device; the bodies' positions widened into the call's scratch
 * (the points: uploaded); sample_sort = 1 (default): the home-cell keys and the stable rocPRIM sort of the deposit, so that
 * neighbouring lanes gather from neighbouring cells; k_sample -- one lane per point of that order, the up to 27 offsets
 * unrolled with constant indices, the grid read through const __restrict__ vector loads, each lane writing its own row, the
 * counts from ballots and one integer atomic per wave and class; no floating-point atomics, no LDS, no lane waits for another.
 * In the gradient ops the stencil cells along the differentiated axis share their reads (TSC order 2: 5 cells, not 6; order
 * 4: 7, not 12).  sample_pregrad = 1 (default 0): k_grid_diff first writes the three difference grids for all cells and
 * k_sample reads them as three fields, recomputing from the indices which terms are dropped; it is treated as 0 when 3 nx ny nz
 * > NBODY_DEPOSIT_MAX_CELLS, and the stats report the plan used.  Nothing chooses a plan for the caller.  nbody_grid_sample_at
 * works through its points in batches of 2^22 after the one copy of the grid.
 *   NOT TIMED ON AN MI355X beyond the single run of tools/sample_bench.py that DESIGN 3.25 records.  Nothing asserts or
 * promises a time.
 *   Accepted and refused on the handles of nbody_deposit.  Refused with NBODY_ERR_INVALID (nbody_last_error names the call):
 * whatever nbody_host_deposit refuses in a spec; fields outside 1 .. 4; fields != 1 with a gradient; an unknown op; fields nx
 * ny nz > NBODY_DEPOSIT_MAX_CELLS; grid NULL; out NULL or xyz NULL with n > 0; n_points > 2^31 - 1; handles of a multi-rank
 * world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without touching a device.
 *   OUT OF SCOPE: a grid component of nbody_set_external_field (a tabulated background in the kick: the natural follow-up, but
 * it touches the step kernels); a device-resident grid kept between calls; PCS stencils;
 * interlacing and deconvolution; multi-rank handles. */
#define NBODY_SAMPLE_VALUE 0      /* the grid's value                                   out [n][fields] */
#define NBODY_SAMPLE_GRADIENT2 1  /* central differences of order 2, fields must be 1   out [n][3]      */
#define NBODY_SAMPLE_GRADIENT4 2  /* central differences of order 4, fields must be 1   out [n][3]      */
#define NBODY_SAMPLE_MAX_FIELDS 4
int nbody_grid_sample(NbodyHandle* h, const NbodyGridSpec* spec, const double* grid /* [fields][nx][ny][nz] */, int fields, int op,
                      double* out, uint8_t* cls /* [n], may be NULL */, size_t cap, size_t* n_out, uint64_t counts[4] /* may be NULL */);
int nbody_grid_sample_at(NbodyHandle* h, const NbodyGridSpec* spec, const double* grid, int fields, int op,
                         const double* xyz /* [n_points][3] */, size_t n_points, double* out, uint8_t* cls, uint64_t counts[4]);
int nbody_host_grid_sample(const double* xyz /* [n][3] */, size_t n, const NbodyGridSpec* spec, const double* grid, int fields, int op,
                           double* out, uint8_t* cls, uint64_t counts[4]);
int nbody_grid_sample_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- grid Poisson: the potential of a mass grid by a hand-written f64 FFT (no reference counterpart) ----------------------
 * What stands between nbody_deposit and nbody_grid_sample in a particle-mesh field: mass is what nbody_deposit returns with
 * NBODY_DEPOSIT_MASS -- mass per cell, not density --, phi the potential at the cell centres; handed to nbody_grid_sample
 * with NBODY_SAMPLE_GRADIENT2 or GRADIENT4 it gives +grad phi.  spec->periodic selects the boundary condition:
 *   PERIODIC (periodic = 1): the Green's function of the continuous Laplacian (NBODY_POISSON_SPECTRAL) or of the 7-point one,
 * the mate of NBODY_SAMPLE_GRADIENT2 (NBODY_POISSON_DIFF2); deconvolve = 0, 1 or 2 divides that many powers of the window of
 * spec->scheme out.  The mean of the mass is removed; the mean of phi is zero.
 *   ISOLATED (periodic = 0): Hockney-Eastwood zero padding -- phi[c] = -g sum_c' mass[c'] Kr(c - c') with Kr = 1 / sqrt(r^2 +
 * soften^2) between cell centres and no self term when soften = 0 -- which a direct sum over the cells reproduces to rounding.
 *   The spec is checked exactly as nbody_host_deposit checks it; in addition every dimension is a power of two.  origin and
 * quantity are ignored, scheme matters only for deconvolve.  An axis of one cell is neither transformed nor padded, so
 * project_axis grids are such grids.  mass and phi may be the same array.  cap = the doubles phi holds; cap < nx ny nz:
 * NBODY_ERR_CAPACITY with phi untouched.
 *   The handle lends its stream and its memory only, as for nbody_grid_sample_at (it may hold no body).  A READ-ONLY call
 * under the contract of nbody_deposit: scratch goes through the handle's registry and is freed inside the call; it leaves no
 * trace in state, stats, tracers or the bits of any later step; the one thing left behind is the record
 * nbody_grid_poisson_stats reads.  nbody_host_grid_poisson is the same arithmetic on the host (no device needed, one thread).
 *   THE ARITHMETIC (csrc/poisson_grid.h, restated in tests/poisson_ref.py), all f64, every operation rounded on its own, nothing
 * contracted into an FMA.  Every output is a fixed expression tree of the inputs -- no sum is longer than a butterfly's two
 * operands -- so THE SAME INPUT GIVES THE SAME BITS on the device, on the host and in the restatement, whatever the launch
 * shape and the poisson_lds and poisson_tile knobs are.
 *     the real grid becomes complex with imaginary parts +0.0.  Per axis of length L = 2^p: the bit-reversal permutation, then
 *     stages s = 1 .. p of radix 2, decimation in time; the butterfly on (a, b) with w = T[j L / 2^s]:
 *         t.re = w.re b.re - w.im b.im;  t.im = w.re b.im + w.im b.re;  a' = a + t;  b' = a - t     (no shortcut for any w)
 *     axis order z, y, x, forward and inverse; the inverse uses (w.re, -w.im); one multiplication by 1 / points at the end.
 *     T[k] = (cos(a), -sin(a)), a = (2 pi k) / L, is made ON THE HOST from std::cos and std::sin and uploaded -- the device
 *     never evaluates a sine, a cosine or a pi --, with T[0] = (1, +0) and T[L / 4] = (+0, -1) written as constants;
 *     nbody_host_poisson_twiddles returns the table of one length (a power of two in 2 .. 4096; else NBODY_ERR_INVALID).
 *     PERIODIC: per axis of n cells, on the host, m = i <= n / 2 ? i : i - n:
 *         SPECTRAL  k = (2 pi m) / (n spacing), K[i] = k k;      DIFF2  v = (2 sin((pi i) / n)) / spacing, K[i] = v v
 *         deconvolve = d > 0:  a = (pi m) / n, s = sin(a) / a, D[i] = 1 / (s multiplied d (scheme + 1) times), D[0] = 1
 *       an axis of one cell has K = 0 and D = 1.  c = -((4 pi g) / ((spacing spacing) spacing)), once.  Per mode
 *         den = (Kx[i] + Ky[j]) + Kz[l];  f = den == 0 ? +0.0 : c / den;  d > 0: f = f ((Dx Dy) Dz);  phi^ = (f rho^.re, f rho^.im)
 *       and phi[cell] = value.re (1 / points) + 0.0.
 *     ISOLATED: every axis of more than one cell is padded to 2 n with +0.0.  On the padded grid Kr = 1 / sqrt(r2), r2 = ((dx dx
 *       + dy dy) + dz dz) + soften soften, d_c = spacing m_c, m_c = i <= n_c ? i : 2 n_c - i (0 on an axis of one cell); at the
 *       origin Kr = soften > 0 ? 1 / soften : +0.0.  sqrt and the division are IEEE on both sides.  Kr goes through the same
 *       transform, each mode is the full complex product in the butterfly's form, and phi[cell] = (-g) (value.re (1 / points))
 *       + 0.0 for the nx ny nz corner.  (The + 0.0: a zero result is +0.0, so an all-zero grid gives +0.0 everywhere.)
 *   nbody_grid_poisson_stats: out = {1 once a call on this handle reached the device else 0, the plan the last such call USED as
 * poisson_lds | lines per block of the strided passes << 1, the butterfly launches, the complex points transformed (points
 * times the 3-D transforms: 2 periodic, 3 isolated)}.  A DIAGNOSTIC AID for tools/poisson_bench.py and the tests of the plans,
 * NOT A STABLE CONTRACT: what the four words mean may change with the kernels.
 *   HOW (csrc/kernels_poisson.hip): one copy of the grid up and one down.  k_poisson_load writes real to complex and pads;
 * k_poisson_kernel fills Kr (isolated only); k_poisson_fft_lds (poisson_lds = 1, the default) -- a block holds whole lines of
 * one axis in LDS, up to 4 096 complex points (64 KB, so one line of the longest axis always fits), reverses the bits on the
 * way in, runs all p stages out of LDS with a barrier between stages and writes back; along the strided axes y and x it takes
 * a tile of poisson_tile (default 16, 1 .. 64, rounded down to a power of two and to what fits) z-adjacent lines, so that
 * global loads and stores stay contiguous along z; the LDS image is padded by one point in 16 and one in 256 against bank
 * conflicts.  poisson_lds = 0: k_poisson_bitrev and one k_poisson_fft_stage launch per stage over global memory, the plain
 * variant and the cross-check.  k_poisson_green (periodic) or k_poisson_mul (isolated), the inverse passes, k_poisson_store
 * (the scale, the corner, -g).  No floating-point atomics.  Nothing chooses a plan for the caller.
 *   COST: 16 bytes per padded point of scratch (32 isolated); every axis pass reads and writes every point once under the LDS
 * plan and p times under the plain one.  NOT TIMED ON AN MI355X beyond the single run of tools/poisson_bench.py that DESIGN
 * 3.26 records.  Nothing asserts or promises a time.
 *   Accepted and refused on the handles of nbody_deposit.  Refused with NBODY_ERR_INVALID (nbody_last_error names the call):
 * whatever nbody_host_deposit refuses in a spec; a dimension that is not a power of two; a padded axis longer than
 * NBODY_POISSON_MAX_AXIS; padded points above NBODY_POISSON_MAX_POINTS; ps NULL; g or soften not finite; soften < 0; soften
 * != 0, green or deconvolve set for the wrong boundary condition; an unknown green; deconvolve outside 0 .. 2; reserved words
 * not 0; mass or phi NULL; handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without
 * touching a device.
 *   OUT OF SCOPE: real-to-complex transforms (the call does twice the necessary work); axes longer than 4 096;
 * non-power-of-two dimensions; a transformed kernel or a device grid kept between calls of nbody_grid_poisson itself
 * (nbody_pm_field below fuses deposit, solve and sample without the host round trips; mesh gravity keeps the kernel and
 * steps with the field); a 4th-order Green's function; interlacing; multi-rank handles. */
#define NBODY_POISSON_SPECTRAL 0   /* periodic: -k^2 of the continuous Laplacian            */
#define NBODY_POISSON_DIFF2    1   /* periodic: the 7-point Laplacian, the mate of GRADIENT2 */
#define NBODY_POISSON_MAX_AXIS   4096        /* transform length of an axis (after padding) */
#define NBODY_POISSON_MAX_POINTS 134217728   /* 2^27 complex points (after padding)         */
typedef struct NbodyPoissonSpec {
    double  g;           /* gravitational constant, finite */
    double  soften;      /* isolated only: epsilon >= 0, finite; must be 0 when periodic */
    int32_t green;       /* periodic only: SPECTRAL | DIFF2; must be 0 when isolated */
    int32_t deconvolve;  /* periodic only: 0, 1 or 2 powers of the spec's scheme window divided out */
    int32_t reserved[2]; /* 0 */
} NbodyPoissonSpec;
int nbody_grid_poisson(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyPoissonSpec* ps,
                       const double* mass /* [nx][ny][nz] */, double* phi /* [nx][ny][nz] */, size_t cap);
int nbody_host_grid_poisson(const NbodyGridSpec* spec, const NbodyPoissonSpec* ps, const double* mass, double* phi, size_t cap);
int nbody_host_poisson_twiddles(int length, double* out /* [length/2][2] */);
int nbody_grid_poisson_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- particle-mesh field: deposit, solve and sample in one call, on the device (no reference counterpart) ------------------
 * The mesh acceleration and potential of the handle's bodies, at the bodies themselves (nbody_pm_field) or at n_points caller
 * points (nbody_pm_field_at): the only O(N + M log M) force of this library, M the cells.  NO NEW ARITHMETIC.  THE DEFINITION
 * is the composition of the three host calls above, byte for byte; with P = the points (the bodies, or xyz):
 *     M    = nbody_host_deposit(bodies, m, spec)                      counts[0..3] = its counts
 *     Phi  = nbody_host_grid_poisson(spec, pm->poisson, M)
 *     grad = nbody_host_grid_sample(P, spec, Phi, 1, pm->gradient)    cls, counts[4..7] = its classes and counts
 *     acc[i][k] = 0.0 - grad[i][k]                                    (so a zero is +0.0)
 *     phi[i]    = nbody_host_grid_sample(P, spec, Phi, 1, NBODY_SAMPLE_VALUE)[i]
 * nbody_host_pm_field is literally that (no device needed; xyz == NULL: P is the bodies and n_points is ignored), and the device
 * calls return these bytes under every plan, on NBODY_F32 and NBODY_F64 handles alike (an NBODY_F32 handle's positions and
 * masses are widened exactly, as in the three calls).  cls is the class of the GRADIENT's sample (the stencil widened by the
 * difference's reach), not the value's.
 *   WHAT A PM FORCE IS AND IS NOT.  Its resolution is about two cells: below that the force falls under Newton's, smoothly for
 * CIC and TSC.  A body feels its own mesh image: its mass is part of M, nothing subtracts it, and phi at a body includes
 * the body's own smeared potential (with soften = 0 on an isolated grid the own cell alone contributes nothing).  Momentum is conserved
 * -- sum m_i acc_i = 0 to rounding -- ONLY BECAUSE deposit and sample share one stencil (deposit_grid.h's), and on a periodic
 * grid; bodies off an isolated grid push and are not pushed.  There is no short-range correction: this is PM, not P3M or TreePM
 * ("P3M field" below adds one on periodic grids).
 *   nbody_pm_field: rows in nbody_download's order, *n_out = the live count; cap = the rows acc (and phi, cls) hold; cap
 * smaller than the live count: NBODY_ERR_CAPACITY with *n_out set and nothing written.  n == 0: NBODY_OK, counts zeroed,
 * nothing else written.  nbody_pm_field_at on a handle that holds no body: every output is +0.0.  phi, cls, n_out and counts
 * may be NULL.
 *   READ-ONLY calls under the contract of nbody_deposit: tracers and the external field play no part; on a Hermite handle the
 * bodies are the held (x0, v0); the live count is read on the device, so a call right after a retain inside unsynchronised
 * nbody_steps is valid; scratch is ONE allocation through the handle's registry, freed inside the call.  A call leaves nothing
 * behind but the record nbody_pm_field_stats reads: the records of nbody_deposit_stats, nbody_grid_sample_stats and
 * nbody_grid_poisson_stats stay as they were.
 *   HOW (csrc/nbody_pm.cpp, csrc/kernels_pm.hip).  One allocation holds the pieces of all three stages; the deposit's int64
 * sums, converted in place to doubles, ARE the Poisson stage's real grid, and after k_poisson_store that grid IS the sampler's:
 * no grid crosses the bus.  The only copies are the Poisson tables up and the rows, classes and words down, with one
 * hipStreamSynchronize at the end (at the bodies a second one, for the live count of the capacity check, as in
 * nbody_grid_sample).  The existing deposit_*, poisson_* and sample_sort knobs are honoured.  Two knobs of its own, which change
 * no result:
 *     pm_share_sort (default 1)  at the bodies, with deposit_sort and sample_sort both on, the home-cell keys and the stable
 *                 rocPRIM sort are made ONCE (the sampler's keys, which depend on the position alone) and used by k_deposit and by
 *                 the gather; 0: two sorts, the cross-check.  nbody_pm_field_at always sorts bodies and points apart.
 *     pm_gather (default 1)  k_pm_gather<kReach, kScheme>: one lane per point in home-cell order, ONE stencil set-up giving acc
 *                 and phi together; each of the four outputs is the very expression tree of the matching k_sample instance
 *                 (csrc/sample_device.h holds the sums both kernels call).  The x component of the gradient reads every stencil
 *                 cell already, so phi costs no further grid read for CIC and TSC (NGP: the own cell, one read; a grid whose
 *                 project_axis is 0: the value's own reads).  phi == NULL skips the value sum and its store.  Counts from
 *                 ballots and one integer atomic per wave and class; no floating-point atomics, no LDS.  0: two k_sample
 *                 launches over the device grid, gradient then value, honouring sample_pregrad, and a negation: the cross-check.
 * nbody_pm_field_at deposits and solves once, then works through its points in the sampler's batches of 2^22.
 *   nbody_pm_field_stats: out = {1 once a call on this handle reached the device else 0, the plan the last such call USED as
 * pm_gather | pm_share_sort << 1 (the second bit only where one sort did serve both), the grid reads of the gather (pm_gather =
 * 0: of the two k_sample launches together), the radix sorts enqueued}.  A DIAGNOSTIC AID for tools/pm_bench.py and the tests
 * of the plans, NOT A STABLE CONTRACT.
 *   COST: the scratch of the three calls less two grids (8 bytes per cell each).  NOT TIMED ON AN MI355X beyond the single run
 * of tools/pm_bench.py that DESIGN 3.27 records.  Nothing asserts or promises a time.
 *   Accepted and refused on the handles of nbody_deposit.  Refused with NBODY_ERR_INVALID (nbody_last_error names the call):
 * whatever nbody_deposit, nbody_grid_poisson or nbody_grid_sample refuses in a spec or a Poisson spec; spec->quantity !=
 * NBODY_DEPOSIT_MASS; pm NULL; a gradient that is not NBODY_SAMPLE_GRADIENT2 or NBODY_SAMPLE_GRADIENT4; reserved words that
 * are not 0; acc NULL with rows to write; xyz NULL with n_points > 0 (the device call); n_points > 2^31 - 1; handles of a
 * multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without touching a device.
 *   OUT OF SCOPE, in this order: a short-range split HERE (nbody_p3m_field below is its own call); real-to-complex transforms; a world-wide mesh energy;
 * multi-rank handles.  (A PM term in the step is "mesh gravity" below, which also keeps an isolated grid's transformed kernel
 * between its passes; nbody_pm_field itself makes it at every call, as before.) */
typedef struct NbodyPmSpec {
    NbodyPoissonSpec poisson;   /* as for nbody_grid_poisson */
    int32_t gradient;           /* NBODY_SAMPLE_GRADIENT2 or NBODY_SAMPLE_GRADIENT4 */
    int32_t reserved[3];        /* 0 */
} NbodyPmSpec;
int nbody_pm_field(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyPmSpec* pm,
                   double* acc /* [n][3] */, double* phi /* [n], may be NULL */, uint8_t* cls /* [n], may be NULL */,
                   size_t cap, size_t* n_out, uint64_t counts[8] /* may be NULL */);
int nbody_pm_field_at(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyPmSpec* pm,
                      const double* xyz /* [n_points][3] */, size_t n_points,
                      double* acc, double* phi, uint8_t* cls, uint64_t counts[8]);
int nbody_host_pm_field(const double* body_xyz, const double* body_m, size_t n_bodies,
                        const NbodyGridSpec* spec, const NbodyPmSpec* pm,
                        const double* xyz /* NULL: the bodies themselves */, size_t n_points,
                        double* acc, double* phi, uint8_t* cls, uint64_t counts[8]);
int nbody_pm_field_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- P3M field: the mesh field plus an exact short-range pair sum (no reference counterpart) ------------------------------
 * The particle-mesh field above resolves about two cells.  nbody_p3m_field (at the bodies) and nbody_p3m_field_at (at n_points
 * caller points) split 1/r with a Gaussian of scale r_split: the mesh carries the smooth long-range part, and a periodic,
 * minimum-image pair sum over the bodies closer than r_cut carries the rest.  PERIODIC GRIDS ONLY.  g is p3m->pm.poisson.g.
 * All of it is f64, every operation rounded on its own, nothing contracted into an FMA (csrc/p3m_pairs.h states it once for the
 * device and the host; tests/p3m_ref.py restates it in numpy).  THE DEFINITION:
 *   MESH PART.  nbody_host_pm_field's composition (above) with one change in the periodic Green stage: the per-axis factor
 * table is D'[i] = D[i] S[i], one product made on the host, S[i] = exp(-(K[i] (r_split r_split))) with the K[i] the stage
 * uses already; D[i] = 1 when deconvolve = 0, so the f = f ((Dx Dy) Dz) branch is always taken.  The device evaluates no
 * exponential, k_poisson_green is unchanged, and nbody_grid_poisson's public spec does not know the split.
 *   SHORT-RANGE PART.  With x = r / r_split, F(x) = erfc(x / 2) + (x / sqrt(pi)) exp(-x^2 / 4) multiplies the Newtonian force and
 * P(x) = erfc(x / 2) the Newtonian potential.  nbody_host_p3m_table tabulates both at x_k = k h, h = (r_cut / r_split) / 4096.0,
 * k = 0 .. 4096, from std::erfc and std::exp:
 *     x = double(k) h;  e = erfc(x / 2.0);  T[k].F = e + (x / SQRT_PI) exp(-((x x) / 4.0));  T[k].P = e
 * SQRT_PI = 1.7724538509055159.  The table is uploaded; the device interpolates linearly and never evaluates erfc.
 *     chain cells  c = the smallest power of two with c spacing >= r_cut.  A body's chain cell is its NGP home cell
 *                  (floor(u_c), u_c = (x_c - origin_c) / spacing, wrapped into [0, dims_c)) shifted right by log2(c) on each axis.
 *                  A body that nbody_deposit SKIPS (x, y, z or m not finite, or !(|u_c| < 2^31)) has no chain cell: it feels and
 *                  exerts no short-range term (its short part is +0.0).  A caller's point takes the same rule with m = 0.0.
 *     partners     of target i: the bodies of the 27 chain cells around its own, visited dx = -1, 0, +1 outermost, then dy, then
 *                  dz innermost, chain indices wrapped; within a cell in ascending row; at the bodies j == i is left out.
 *     term         d_c = x_j,c - x_i,c, then d_c = d_c - rint(d_c / L_c) L_c with L_c = double(dims_c) spacing;
 *                  r2 = (dx dx + dy dy) + dz dz.  The term counts iff r2 < R2 STRICTLY, R2 = r_cut r_cut, and is skipped when
 *                  r2 == 0 and soften == 0.  r = sqrt(r2), t = r (4096.0 / r_cut), k = min((int) t, 4095), fr = t - double(k);
 *                  Fv = T[k].F + fr (T[k + 1].F - T[k].F), Pv likewise;  s2 = r2 + soften soften, inv = 1.0 / sqrt(s2),
 *                  inv3 = (inv inv) inv.
 *     sums         ax, ay, az, ph start at +0.0 and run in that one sequential order:  a_c = a_c + ((m_j inv3) Fv) d_c,
 *                  ph = ph + (m_j inv) Pv.  At the end acc_short_c = g a_c and phi_short = 0.0 - g ph.
 *   TOTAL.  acc = acc_mesh + acc_short and phi = phi_mesh + phi_short, one addition each.  NBODY_P3M_MESH_ONLY and
 * NBODY_P3M_SHORT_ONLY return the one part (diagnostic: both still run the mesh stages, because cls and counts are the MESH
 * PART's under every value of terms).  THE ORDER IS PART OF THE DEFINITION: it depends on the state and the spec only, never on
 * the launch shape, so the device (under both plans), the host and the restatement give the same bits, on NBODY_F32 and
 * NBODY_F64 handles alike (positions and masses widened exactly).
 *   PHYSICS.  phi at a body still contains the body's own long-range image, -g m / (r_split sqrt(pi)), as nbody_pm_field's
 * contains its smeared image; nothing subtracts it.  r2, the table index and d are exactly antisymmetric in (i, j), so
 * sum m_i acc_short_i vanishes to rounding.  The walk sees every pair whose minimum-image distance is below r_cut, up to the
 * rounding of u at cell faces: DESIGN 3.30 states and proves the margin.
 *   Argument shapes, the NULL rules, the capacity rule, the n == 0 rule, cls and counts are nbody_pm_field's, word for word, and
 * so is the READ-ONLY contract: scratch is ONE allocation through the handle's registry, freed inside the call; a call leaves
 * nothing behind but the record nbody_p3m_field_stats reads -- the records of nbody_pm_field_stats, nbody_deposit_stats,
 * nbody_grid_sample_stats and nbody_grid_poisson_stats stay as they were.
 *   HOW (csrc/nbody_p3m.cpp, csrc/kernels_p3m.hip).  The mesh stages are nbody_pm_field's own, reused with their knobs; no
 * grid crosses the bus.  The bodies are keyed by chain cell, ordered by the stable rocPRIM sort the grid calls use, gathered
 * into that order as {x, y, z, m}, and a dense cell-start table is made by binary search (the chain grid has at most
 * (dims / c)^3 cells).  k_p3m_short<kAtPoints, kLds>: one block of 128 lanes per chain cell (a block whose cell holds no target
 * leaves at once); lanes own the cell's targets, in tiles of 128 when it holds more; the partner stream of the 27 cells is
 * staged through LDS in the defined order as position, mass and row, and every lane runs the same sequential sums.  The pair
 * counts are integers formed on the device.  No floating-point atomics.  One synchronisation at the end (at the bodies a second
 * one, for the live count, as in nbody_pm_field).  nbody_p3m_field_at orders its points by their own chain cell, has no self
 * term and works in the sampler's batches.  One knob, which changes no result:
 *     p3m_lds (default 1)  0: one lane per target reading the partners from global memory, the plain variant and cross-check
 *   nbody_p3m_field_stats: out = {1 once a call on this handle reached the device else 0, the plan of the last such call as
 * p3m_lds | (nbody_pm_field_stats's plan word) << 1, the partners looked at (self left out), the terms with r2 < R2}; the two
 * pair counts depend on the state and the spec only.  A DIAGNOSTIC AID, NOT A STABLE CONTRACT.
 *   NOT TIMED ON AN MI355X beyond the single run of tools/p3m_bench.py that DESIGN 3.30 records.  Nothing asserts or promises a
 * time.
 *   Refused with NBODY_ERR_INVALID (nbody_last_error names the call): whatever nbody_pm_field refuses; p3m NULL; a grid that is
 * not periodic; project_axis != -1; any dims_c / c < 4 (the three neighbour cells on an axis must be distinct); r_split not
 * finite or <= 0; r_cut not finite or outside r_split .. 8 r_split; soften not finite or < 0; an unknown terms; reserved != 0;
 * handles of a multi-rank world and NBODY_SHARD_SPATIAL handles.  A NULL handle is refused without touching a device.
 * nbody_host_p3m_table refuses the same r_split and r_cut and a NULL out.
 *   OUT OF SCOPE: P3M in the step; isolated grids; TreePM; subtracting the self image from phi; a mesh energy; optimal
 * (Hockney-Eastwood) influence functions and interlacing; multi-rank handles. */
#define NBODY_P3M_TABLE_INTERVALS 4096
enum { NBODY_P3M_BOTH = 0, NBODY_P3M_MESH_ONLY = 1, NBODY_P3M_SHORT_ONLY = 2 };
typedef struct NbodyP3mSpec {
    NbodyPmSpec pm;      /* as for nbody_pm_field; periodic grids only */
    double  r_split;     /* r_s > 0, finite: the Gaussian split scale, a length */
    double  r_cut;       /* finite, r_split <= r_cut <= 8 r_split: short-range terms end here */
    double  soften;      /* Plummer epsilon >= 0 of the short-range term, finite */
    int32_t terms;       /* NBODY_P3M_BOTH, NBODY_P3M_MESH_ONLY or NBODY_P3M_SHORT_ONLY */
    int32_t reserved;    /* 0 */
} NbodyP3mSpec;
int nbody_p3m_field(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyP3mSpec* p3m,
                    double* acc /* [n][3] */, double* phi /* [n], may be NULL */, uint8_t* cls /* [n], may be NULL */,
                    size_t cap, size_t* n_out, uint64_t counts[8] /* may be NULL */);
int nbody_p3m_field_at(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyP3mSpec* p3m,
                       const double* xyz /* [n_points][3] */, size_t n_points,
                       double* acc, double* phi, uint8_t* cls, uint64_t counts[8]);
int nbody_host_p3m_field(const double* body_xyz, const double* body_m, size_t n_bodies,
                         const NbodyGridSpec* spec, const NbodyP3mSpec* p3m,
                         const double* xyz /* NULL: the bodies themselves */, size_t n_points,
                         double* acc, double* phi, uint8_t* cls, uint64_t counts[8]);
int nbody_host_p3m_table(double r_split, double r_cut, double* out /* [4097][2] = {F, P} */);
int nbody_p3m_field_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- mesh gravity: the particle-mesh field as the self-gravity of the step (no reference counterpart) --------------------
 * nbody_set_mesh_gravity(h, spec, pm): while set, the self-gravity pass of every step and of nbody_update_forces IS the mesh
 * field of nbody_pm_field; no pair kernel is launched.  spec == NULL and pm == NULL: off.  NO NEW ARITHMETIC.  THE DEFINITION:
 * with x the half-drifted, retained positions P of the live bodies and their masses m, widened exactly, and g the handle's g as
 * it stands at the pass, widened exactly,
 *     acc_pass[i][c] = F( nbody_host_pm_field(P, m, spec, pm with poisson.g := g).acc[i][c] )
 * F = one IEEE round-to-nearest-even conversion to the handle's dtype (the identity on NBODY_F64 handles).  pm->poisson.g is
 * NOT READ by a pass (nbody_get_mesh_gravity returns it as set); g_soft plays no part: the mesh's softening is
 * pm->poisson.soften.  Bodies off an isolated grid get +0.0, as nbody_pm_field gives them.
 *   THE STEP is otherwise unchanged: half drift, retain, this pass, then kick_half_drift's arithmetic -- v += a dt; x += (v 0.5)
 * dt, every product rounded on its own.  With an external field set, acc = acc_pass + s(x), exactly as "external field"
 * states it.  Tracers get the same mesh field at their own half-drifted, retained positions: nbody_host_pm_field with xyz = the
 * tracers, rounded by F.  nbody_steps(k) gives the bits of k nbody_step_by calls; nbody_clone carries the setting.
 *   WHAT DOES NOT CHANGE: a handle that never sets mesh gravity runs the code it ran before; one that sets and clears it with no
 * pass in between gives the bits of one that never did.  nbody_energy*, nbody_potentials, nbody_field_at, nbody_pm_field and
 * every diagnostic call stay as they are (all-pairs self-gravity, or the mesh call's own spec).  NbodyStats.steps counts as
 * before; the interaction counters do not move during mesh passes.
 *   HOW (csrc/nbody_mesh.cpp, csrc/kernels_mesh.hip).  The handle keeps ONE particle-mesh scratch through its registry, made at
 * the first pass, remade only when the spec or the bound on the bodies or tracers outgrows it, freed on clear and on destroy.
 * It holds the Poisson tables, sent once, and on an isolated grid the transformed kernel, which depends on dims, spacing and
 * soften only (-g is applied where phi is written): made once per spec, so a pass does two 3-D transforms, not three, and the
 * expression tree of every output is nbody_pm_field's.  A pass is ENQUEUE-ONLY: no synchronisation, no allocation, no
 * read-back; the live count is read on the device and the launches are sized from the host's bound.  Its last stage is
 * k_mesh_kick<F, kReach, kScheme>: one lane per body in the shared home-cell order, the stencil set-up and gradient sums of
 * k_pm_gather, 0.0 - grad rounded once to F into the acc row, and -- inside a step without an external field -- the kick and
 * half drift of the row; no phi, no f64 rows, no LDS, no floating-point atomics.  Two knobs, which change no result:
 *     mesh_kick_fuse (default 1)    0: nbody_pm_field's gather to f64 rows, a rounding kernel and the leapfrog's own kick
 *     mesh_keep_kernel (default 1)  0: the transformed kernel is made at every pass
 * The deposit_*, sample_sort, poisson_*, pm_share_sort and (with mesh_kick_fuse = 0) pm_gather and sample_pregrad knobs are
 * honoured.
 *   nbody_mesh_gravity_stats: out = {passes enqueued, the plan the last pass used as mesh_kick_fuse | mesh_keep_kernel << 1 |
 * (nbody_pm_field_stats's plan word) << 2, 3-D transforms enqueued in total, allocations of the resident state so far}.  A
 * DIAGNOSTIC AID for tools/mesh_bench.py and the tests of the plans, NOT A STABLE CONTRACT.
 *   ACCEPTED on NBODY_BRUTE_FORCE handles with world_size == 1 (NBODY_SHARD_INDEX), the leapfrog, both dtypes and both math modes
 * (the mesh pass has one arithmetic), with or without tracers and an external field.  REFUSED with NBODY_ERR_INVALID
 * (nbody_last_error names the call; the handle keeps working): whatever nbody_pm_field refuses in a spec or a PM spec;
 * NBODY_BARNES_HUT handles (their unsynchronised-step accounting is out of scope); multi-rank and NBODY_SHARD_SPATIAL handles;
 * exactly one of spec and pm NULL; setting mesh gravity while NBODY_INTEGRATOR_HERMITE4 is selected, and selecting Hermite
 * while mesh gravity is set.
 *   OUT OF SCOPE: Barnes-Hut handles under the mesh; TreePM or P3M short-range terms; Hermite; a mesh energy; multi-rank
 * handles.  NOT TIMED beyond what DESIGN 3.28 records.  Nothing asserts or promises a time. */
int nbody_set_mesh_gravity(NbodyHandle* h, const NbodyGridSpec* spec, const NbodyPmSpec* pm);   /* spec == NULL and pm == NULL: off */
int nbody_get_mesh_gravity(const NbodyHandle* h, NbodyGridSpec* spec, NbodyPmSpec* pm, int* on);
int nbody_mesh_gravity_stats(NbodyHandle* h, uint64_t out[4]);
/* ---- pair search: how the fixed-radius calls find their pairs (no reference counterpart) --------------------------------
 * nbody_fof_labels, nbody_fof_groups, nbody_contacts, nbody_merge_contacts, nbody_neighbors_within, nbody_density,
 * nbody_density_center and nbody_pair_counts ask a FIXED-RADIUS question: only bodies closer than the linking length, the
 * radius or the last bin edge can matter.  nbody_set_pair_search selects how these eight calls find such pairs; nothing else
 * reads the setting as they do (nbody_nearest, nbody_partners and nbody_bound_pairs are not fixed-radius and stay all-pairs;
 * nbody_pair_counts_at always looks at all pairs).  nbody_knn, nbody_knn_density and nbody_knn_density_center ask no
 * fixed-radius question either, but read the setting through their radius_hint: under NBODY_SEARCH_CELLS and with a hint > 0
 * they draw the grid for that length, answer from the 27 cells every row that finds its k bodies inside the hint, and answer the
 * other rows by the all-pairs pass -- the result is the same bits whatever the mode and the hint are; with radius_hint == 0 or
 * under NBODY_SEARCH_ALL_PAIRS they look at all pairs and leave the record behind nbody_pair_search_stats as it was.
 *   NBODY_SEARCH_ALL_PAIRS (the default) is the code as it stands: a handle that never sets the mode runs it untouched.
 *   NBODY_SEARCH_CELLS sorts the bodies by the cell of a uniform grid and looks at the 27 surrounding cells only.  THE GRID IS
 * NOT A TREE -- one level, cells of one size, no opening criterion, nothing approximated -- AND IT CHANGES NO RESULT: all four
 * calls return exactly what they return under NBODY_SEARCH_ALL_PAIRS.  Labels, group counts, member lists and contact lists are
 * equal integer for integer; the seven sums of each group and every NbodyContact field are equal BIT FOR BIT; the state after
 * nbody_merge_contacts is equal bit for bit.  Every other clause of those calls' contracts holds as written (read-only calls
 * leave no trace, the live count is read on the device, scratch goes through the handle's registry and is freed inside the
 * call, no floating-point atomics, the same state gives the same bits).  The record behind nbody_pair_search_stats is the only
 * new thing a call leaves behind.
 *   THE GRID (csrc/cell_grid.h, restated in tests/cells_ref.py), all f64, every operation rounded on its own:
 *     a body is GRIDDED iff its three coordinates are finite (an NBODY_F32 handle's are widened exactly);
 *     lo_c, hi_c = min and max of the gridded bodies' coordinate c (a zero bound counts as +0.0);  E = max_c (hi_c - lo_c);
 *     side = max(length * (1 + 2^-20), E * 2^-20)         (length: the linking length, the radius or |edges[n_bins]| of the call)
 *     k_c  = min((uint64) floor((x_c - lo_c) / side), 2^21 - 1);   key = k_x << 42 | k_y << 21 | k_z
 *     usable = isfinite(E) && isfinite(side) && isfinite(length * length)
 * A CANDIDATE PAIR is an unordered pair of gridded bodies whose cell indices differ by at most 1 on every axis.  Every pair
 * with r2 < length * length in the calls' own rounded arithmetic is a candidate pair (DESIGN 3.19 has the proof); a body that
 * is not gridded has r2 = NaN or +inf to everybody, so it links to and touches nobody under either mode.
 *   FALLBACK RULE: if the grid is not usable (coordinates near +-1e308, say) or no body is gridded, the call runs the
 * all-pairs pass and the record reads {0, 0, 0, 0}.
 *   nbody_set_pair_search may be called at any time between calls; setting a mode and setting it back without a call in
 * between leaves no trace.  nbody_clone carries the mode; the clone's record starts at zero.
 *   nbody_pair_search_stats: out = {1 if the last of the four calls on this handle ran the cell search, else 0; bodies gridded;
 * occupied cells (distinct keys); candidate pairs}.  Integers formed on the device; they depend on the state and the length
 * only, not on the launch shape.  A call that returns before any pair is looked at (no bodies; nbody_fof_labels with label
 * and n_groups_out both NULL) leaves the record as it was.
 *   nbody_host_cell_grid (host only, no device needed): the grid this library would draw for n points {x, y, z} and a length
 * (finite and > 0, else NBODY_ERR_INVALID): lo, side, usable and -- key != NULL -- every point's key (all ones for a point
 * that is not gridded, and for every point when the grid is not usable).  With no gridded point lo = 0 and E = 0.
 *   COST: O(N log N) for the radix sort of (key, row) and the binary searches that find a column of cells among the sorted
 * keys, plus one f64 pair term per candidate pair (nbody_contacts: two, one from either side).  One cell holding every body
 * is legal and merely slow.  NOT MEASURED on an MI355X beyond the single run of tools/cells_bench.py that the table of DESIGN
 * 3.19 records; nothing asserts or promises a time, and nothing chooses a mode for the caller.
 *   Accepted wherever nbody_fof_labels is accepted.  Refused with NBODY_ERR_INVALID (all three handle calls; nbody_last_error
 * names the call): a mode other than 0 or 1; handles of a multi-rank world; NBODY_SHARD_SPATIAL handles.  A NULL handle is
 * refused without touching a device. */
enum { NBODY_SEARCH_ALL_PAIRS = 0,  /* default: every pair is looked at */
       NBODY_SEARCH_CELLS = 1 };    /* the 27 cells around a body's own */
int nbody_set_pair_search(NbodyHandle* h, int mode);
int nbody_get_pair_search(const NbodyHandle* h, int* mode);
int nbody_pair_search_stats(NbodyHandle* h, uint64_t out[4]);
int nbody_host_cell_grid(const double* xyz, size_t n, double length, double lo[3], double* side, uint64_t* key /* [n], may be NULL */,
                         int* usable);
const char* nbody_last_error(const NbodyHandle* h); /* h may be NULL: last create/clone error */

/* ---- launch-shape and scheme knobs of one handle (no reference counterpart) --------------------------------- */
/* Per handle; the library exports no mutable globals.  Names (csrc/kernels.h struct Tuning): cross_sym, sym_packed,
 * bf_fast_variant, sym_wpb, sym_rounds, sym_reduce_split, sym_opp_rot, cross_slots, cross_ipt, cross_wpb, bh_walk_split, bh_walk_order,
 * bh_reduce_split, tree_max_tie, bf64_min_bodies, bf64_ipt, bf64_rot, bf64_waves (f64 fast brute force; a Hermite handle's pair-jerk pass reads bf64_ipt as 4 unless it is 8),
 * pair_hist_combine, pair_hist_flush (nbody_pair_counts and nbody_pair_counts_at: they change no result), deposit_sort, deposit_combine,
 * deposit_lds (nbody_deposit: the plan, defaults 1, 1, 1; they change no result), sample_sort, sample_pregrad (nbody_grid_sample and
 * nbody_grid_sample_at: the plan, defaults 1, 0; they change no result), poisson_lds, poisson_tile (nbody_grid_poisson: the plan,
 * defaults 1, 16; they change no result), pm_gather, pm_share_sort (nbody_pm_field and nbody_pm_field_at: the plan, defaults 1, 1; they
 * change no result), p3m_lds (nbody_p3m_field and nbody_p3m_field_at: the plan, default 1; it changes no result), mesh_kick_fuse, mesh_keep_kernel (mesh gravity: the plan, defaults 1, 1; they change no result); the
 * environment switches NBODY_CROSS_SYM, NBODY_SYM_PACKED, NBODY_BF_VARIANT, NBODY_SYM_WPB
 * and NBODY_BH_SPLIT preset them at nbody_create.  cross_sym, sym_packed and bf_fast_variant are part of what the ranks of a
 * world agree on at nbody_comm_init and cannot change afterwards.  bh_walk_variant, bh_walk_lds_block, bh_hot_cap,
 * bh_walk_debug and sym_debug select experimental walks and in-kernel stamps that only the tuning build carries
 * (libnbody_hip_tuning.so, `make -C nbody-llm_amd/csrc tuning`): the release library refuses them. */
int nbody_set_tuning(NbodyHandle* h, const char* name, int value);
int nbody_get_tuning(const NbodyHandle* h, const char* name, int* value);
int nbody_is_tuning_build(void);

/* ---- multi-GPU (no reference counterpart) ------------------------ */
#define NBODY_COMM_ID_BYTES 128
/* rank 0 calls nbody_comm_unique_id and ships the bytes to the other ranks out of band; every
 * rank then calls nbody_comm_init on its handle (collective).  The id names the transport of the exchanges:
 *   nbody_comm_unique_id  RCCL (one process per GPU, xGMI) -- or, with NBODY_TRANSPORT=ipc in the environment, the same
 *                         as nbody_comm_local_id;
 *   nbody_comm_local_id   ranks that share ONE device (processes, or threads of one process, on the same host): payloads
 *                         staged through hipIpc-shared windows, flags in host shared memory (csrc/transport_ipc.hip).
 *                         RCCL refuses two ranks on one device; this is how the multi-rank step runs on a one-GPU box.
 * nbody_comm_init also checks that every rank was created alike (ABI version, method, arithmetic, sharding, capacity,
 * exchange scheme): a rank that differs gets NBODY_ERR_COMM there instead of a hang in the first exchange. */
int nbody_comm_unique_id(void* id_bytes);
int nbody_comm_local_id(void* id_bytes);
int nbody_comm_init(NbodyHandle* h, const void* id_bytes);
/* "rccl", "ipc" or "none" */
int nbody_comm_transport(const NbodyHandle* h, char* out, size_t cap);
/* first global index and length of this rank's block at upload time */
int nbody_local_range(const NbodyHandle* h, size_t* first, size_t* count);
/* NBODY_SHARD_SPATIAL: a rank's bodies are not an index block (and change as bodies migrate).  This gives, in the
 * order nbody_download writes the bodies, each one's index in the uploaded vector: scattering all ranks' bodies by it
 * restores the reference's vector order (Vec::retain keeps relative order, so the indices stay ascending there). */
int nbody_download_ids(NbodyHandle* h, int32_t* ids, size_t cap, size_t* n_out);
typedef struct NbodyLetStats {
    uint64_t steps;             /* force passes counted */
    uint64_t bodies_migrated;   /* bodies this rank sent to another rank */
    uint64_t nodes_local;       /* nodes of this rank's slice, summed over the passes */
    uint64_t nodes_global;      /* nodes of the whole tree, summed */
    uint64_t nodes_sent;        /* node records this rank exported, summed over partners and passes */
    uint64_t nodes_received;    /* node records it imported */
    uint64_t bytes_sent;        /* bytes of all four exchanges this rank sent (migrants, end info, spanning-cell tables, nodes) */
    uint64_t bytes_allgather_equivalent; /* what the index-block scheme sends per rank for the same passes: 16 B per own body */
    double phase_ms[5];         /* device time of the five phases between the exchanges, summed over the passes made with
                                 * nbody_set_profiling(h, 1): drift + retain + pick migrants | take them in, keys, sort |
                                 * emit the slice + spanning-cell table | finish + flag + pack the export | walk + kick */
    uint64_t host_syncs;        /* host synchronisations inside the passes (steady state: one per pass, where the export counts are read) */
    uint64_t migrant_respills;  /* passes whose migrants did not fit the sizes their messages were posted with and made the round twice */
    uint64_t node_array_peak_bytes;  /* most bytes of node records this rank held at once: its own slice + what it imported */
    uint64_t node_array_bytes;       /* bytes of every buffer of node records this rank has allocated: its slice, the array the walk runs over
                                        (slice + imports, in global-index order), the export lists, the staged imports -- sized from the
                                        rank's own capacity, not from the world's */
} NbodyLetStats;
int nbody_let_stats(NbodyHandle* h, NbodyLetStats* out);

/* ---- synthetic initial conditions (host side; what src/main.rs:52-89 does for the disc) ----- */
/* Plummer sphere, G = M = 1, Henon units, equal masses 1/n, centre of mass at rest at the origin. */
int nbody_ic_plummer(void* aos, size_t n, size_t stride_bytes, uint64_t seed);
/* The reference's self-gravitating disc: 1 unit-mass star + n disc bodies (src/main.rs:52-89);
 * writes n+1 records. */
int nbody_ic_disc(void* aos, size_t n_disc, size_t stride_bytes, uint64_t seed);
/* the same sets as PointParticle<f64,3> records (80 bytes), unrounded */
int nbody_ic_plummer_f64(void* aos, size_t n, size_t stride_bytes, uint64_t seed);
int nbody_ic_disc_f64(void* aos, size_t n_disc, size_t stride_bytes, uint64_t seed);

/* ---- test hooks: one sharded step with the exchange done by the caller ------------------------- */
/* G handles of one process (rank r of world G, same device) stand in for G GPUs: step_begin on
 * each, import every peer's segment into each (the all-gather of positions), step_forces on each,
 * import every peer's partial sums into each (the ncclSend/ncclRecv round of the symmetric scheme
 * across shards; a no-op for force passes that exchange nothing), step_end on each --
 * nbody_step_by with the RCCL transfers replaced by device-to-device copies. */
int nbody_debug_step_begin(NbodyHandle* h, float dt);
int nbody_debug_import_segment(NbodyHandle* h, NbodyHandle* peer);
int nbody_debug_step_forces(NbodyHandle* h, float dt);
int nbody_debug_import_partials(NbodyHandle* h, NbodyHandle* peer);
int nbody_debug_step_end(NbodyHandle* h, float dt);
/* the same for NBODY_SHARD_SPATIAL handles: phases 0..4 of a step (drift + retain + pick migrants | take migrants in +
 * sort | emit the slice + spanning-cell table | finish the spanning cells + pick and pack the nodes partners need |
 * place imports + walk + kick), and between them the four exchanges as copies from `peer` (which = 0 migrants,
 * 1 end info, 2 spanning-cell tables, 3 nodes).  prune = 0 in nbody_debug_let_set_prune exports every private node. */
int nbody_debug_let_phase(NbodyHandle* h, int phase, float dt);
int nbody_debug_let_exchange(NbodyHandle* h, NbodyHandle* peer, int which);
/* by_work = 1 (default): the redrawn bounds give every rank the same share of the last walk's node visits; 0: of the bodies */
int nbody_debug_let_set_balance(NbodyHandle* h, int by_work);
/* the key-range bounds the next classification will use ([world_size + 1]; redrawn every step at the world's quantiles) */
int nbody_debug_let_bounds(NbodyHandle* h, unsigned long long* out);
int nbody_debug_let_set_prune(NbodyHandle* h, int prune);
/* The node array this rank's last force pass (a step's, or nbody_update_forces') walked, in the walk's order: its slice and
 * the imports in the order of their global pre-order indices.  Per held node: com_mass {x, y, z, m}; width; link = the
 * position in this array the walk goes to when it accepts the node or passes it by (a leaf's is its own position + 1; the
 * array's length ends the walk); global_index = its index in the world's pre-order node array; leaf = 1 for a body's leaf;
 * origin = 0 a private node of this rank's slice, 1 a private node imported from a partner, 2 a spanning cell of this
 * rank's slice, 3 an imported spanning cell.  Arrays hold `cap` nodes (com_mass: 4 floats a node) and may each be NULL;
 * all NULL counts only; fewer than *n_nodes: NBODY_ERR_CAPACITY.  NBODY_ERR_INVALID on handles that are not
 * NBODY_SHARD_SPATIAL and before the first force pass after an upload.  Reads only: the state, nbody_stats, nbody_let_stats
 * and the bits of later steps are what they would be without the call. */
int nbody_debug_let_export_held(NbodyHandle* h, float* com_mass, float* width, int32_t* link, int32_t* global_index, int32_t* leaf,
                                int32_t* origin, size_t cap, size_t* n_nodes);

/* ---- host-only entry (no device needed): the plan of the symmetric scheme across shards ---------- */
/* Which pairs between shards `rank` evaluates (rows {shard, first chunk, last chunk, first own set,
 * last own set} of 64-body chunks and 64*ipt-body sets) and which ranks send it partial sums. */
int nbody_host_cross_plan(int rank, int world, int seg_cap, int n_own, int* ipt, int* n_sets, int* n_parts, int* parts,
                          int* n_recv, int* recv_from);

/* ---- host-only entry (no device needed): message layout of the spatial step's variable-size rounds ---- */
/* matrix[r * world + q] = records rank r sends to rank q (all-gathered, the same on every rank).  For `rank`: out_at / n_out
 * [world] = record offset (in its packed send buffer, or q * send_stride when !packed_send) and count of the message to
 * each rank; in_at / n_in [world] = offset in its receive buffer and count of the message from each rank; counts are
 * clamped to `clamp` on BOTH sides of every pair (the byte counts of a send and of the receive that meets it are the
 * same expression). */
int nbody_host_exchange_layout(const int* matrix, int world, int rank, long long clamp, int packed_send, size_t send_stride,
                               size_t* out_at, size_t* n_out, size_t* in_at, size_t* n_in, size_t* total_in);

/* ---- host-only entry (no device needed): the launch shapes the library derives from a body count ---- */
/* With the default knobs: the fast Barnes-Hut walk's bodies per lane and node-range segments for `n_bodies` walked bodies at
 * opening angle theta2 (kernels.h walk_plan), and the symmetric brute-force kernel's bodies per lane of a resident set
 * (sym_bodies_per_lane).  What tools and tests read the plan with; out[0..2] = {walk bodies per lane, walk segments, sym
 * bodies per lane}. */
int nbody_host_launch_plan(size_t n_bodies, float theta2, int fast_math, int out[3]);

/* ---- host-only entry (no device needed): the octree build alone ------------------------------ */
/* BarnesHutSimulation::build_tree (barnes_hut.rs:143-183) + linearisation, as the Barnes-Hut step
 * runs it.  pos4 = n records {x,y,z,m}.  Output arrays hold `cap` nodes (com_mass: 4 floats per
 * node) and may be NULL to count; `order` receives the n body ids in depth-first leaf order. */
int nbody_host_build_tree(const float* pos4, size_t n, const float center[3], float width, int threads,
                          float* com_mass, float* node_width, int32_t* skip, int32_t* leaf_body, int32_t* order,
                          size_t cap, size_t* n_nodes);

int nbody_abi_version(void);
int nbody_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_H */

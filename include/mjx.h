/*
 * mjx.h — C ABI of the MI355X majority-dynamics engine (libmjx.so).
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t
 * passed as `void*` (NULL = the default stream).  Nothing here allocates,
 * synchronises the device or throws: errors come back as an int status
 * (MJX_OK = 0).  Kernels are hand-written HIP for gfx950.
 *
 * Reference interfaces replaced (paths relative to the thesis repository
 * MarekJankola/Master-Thesis-Optimizing-Initialization-in-Graph-Dynamics-
 * from-Ferromagnetism-to-Opinion-Consensus, "nb" = code/ER_BDCM_entropy.ipynb
 * cited by raw JSON line):
 *
 *   onestep_majority(N, s0)      code/SA_RRG.py:18-20, code/HPR_pytorch_RRG.py:169-171
 *   s_endstate(N, s0, p, c)      code/SA_RRG.py:23-26, code/HPR_pytorch_RRG.py:174-177
 *   onestep_majority (ER)        nb:113-117,  s_endstate (ER) nb:120-123
 *   m(s)                         code/SA_RRG.py:39-40, code/HPR_pytorch_RRG.py:179-180, nb:125-126
 *   E_delta + SA loop body       code/SA_RRG.py:32-37, 63-88
 *   HPr_dp, marginals_comp, new_biases_i   code/HPR_pytorch_RRG.py:137-218
 *   BDCM_ER, Zi_ER, Zij, phi/m_init sums   nb:133-276, 372-392
 *
 * Spin layouts in HBM (bit = 1 means spin +1, bit = 0 means spin -1):
 *
 *   node-packed ("np", one replica): word v>>6, bit v&63 holds node v.
 *       n_words = ceil(n/64).
 *   replica-packed ("rp", R = 64*W replicas): word v*W + (r>>6), bit r&63
 *       holds node v of replica r.  One node's W words are contiguous, so a
 *       neighbour gather moves 8*W contiguous bytes.
 *
 * Adjacency:
 *   ELL (random regular graphs): int32 adj[n*d], row v = neighbours of v
 *       (the reference's `N` array, code/SA_RRG.py:9-16).
 *   CSR (Erdos-Renyi): int64 row_ptr[n+1], int32 col[nnz].
 */
#ifndef MJX_H
#define MJX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define MJX_OK        0
#define MJX_EINVAL    1   /* bad argument (size, degree, null pointer ...) */
#define MJX_EHIP      2   /* a HIP runtime call failed                     */
#define MJX_ERANGE    3   /* size outside what the kernels support         */

/* element types for pack/unpack of +-1 spin arrays */
#define MJX_I8   1
#define MJX_I32  4
#define MJX_I64  8
/* floating-point element types (HPR / BDCM message arrays) */
#define MJX_F32  104
#define MJX_F64  108

int         mjx_abi_version(void);            /* bumps on any signature change */
/* Content hash of the sources (csrc/, include/mjx.h) the library was built
 * from; the Python loader refuses a library whose id differs from its tree. */
const char* mjx_build_id(void);
const char* mjx_strerror(int status);
const char* mjx_last_hip_error(void);         /* text of the last failing HIP call */

/* ---- pack / unpack between +-1 integer arrays and bit layouts ----------- */
/* s: (n,) +-1 of element type `dtype` -> node-packed bits[ceil(n/64)] */
int mjx_pack_np(const void* s, int dtype, int64_t n, uint64_t* bits, void* stream);
int mjx_unpack_np(const uint64_t* bits, int64_t n, void* s, int dtype, void* stream);
/* s: (R, n) row-major +-1 (replica r = row r) -> replica-packed bits[n*W],
 * W = ceil(R/64); padding replicas are written as -1 (bit 0).            */
int mjx_pack_rp(const void* s, int dtype, int64_t n, int64_t R, uint64_t* bits, void* stream);
int mjx_unpack_rp(const uint64_t* bits, int64_t n, int64_t R, void* s, int dtype, void* stream);

/* ---- majority rollout (M1 repeated `steps` times, M2) ------------------ */
/*
 * s_out = onestep^steps(s_in).  For steps >= 2 `tmp` must hold a buffer of
 * the same size as s_in (ping-pong); it may be NULL when steps <= 1.
 * s_in may not alias s_out or tmp.  steps == 0 copies.
 * counts (nullable): per-replica number of +1 spins in s_out, ADDED into
 * counts[R] (uint64; caller zeroes it) — the popcount is fused into the last
 * sweep.  For the np layout R = 1 and counts[0] receives the total.
 */
int mjx_rollout_ell_np(const int32_t* adj, int64_t n, int d,
                       const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                       int steps, unsigned long long* counts, void* stream);
int mjx_rollout_ell_rp(const int32_t* adj, int64_t n, int d, int64_t words,
                       const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                       int steps, unsigned long long* counts, void* stream);
/* mjx_rollout_ell_rp with a graph per replica: R replicas in W = ceil(R/64)
 * words per node; replica r (bit r&63 of word column r>>6) runs on graph
 * rep_graph[r] (device int32[R]) of a stack of graphs, graph g's rows at
 * adj + g*n*d; padding replicas (r >= R) are written as -1 (bit 0).  counts
 * (nullable): [R], added.  The reference's SA draws one graph per replica
 * (code/SA_RRG.py:58-62). */
int mjx_rollout_ell_rp_multi(const int32_t* adj, int64_t n, int d, int64_t R, const int32_t* rep_graph,
                             const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                             int steps, unsigned long long* counts, void* stream);
/* The replica-packed rollout run slice by slice: slice q of S covers word units
 * [q*U/S, (q+1)*U/S) of every node (U = words/2 16-byte units, or words if
 * odd); replicas never interact, so the result is identical for every S.
 * slices = 0 follows mjx_rollout_ell_rp_plan (mjx_rollout_ell_rp uses that).
 * S must divide U (MJX_EINVAL otherwise). */
int mjx_rollout_ell_rp_sliced(const int32_t* adj, int64_t n, int d, int64_t words,
                              const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                              int steps, int slices, unsigned long long* counts, void* stream);
/* The same rollout over a slice-major intermediate state: the states between
 * the sweeps are kept as [S][n][words/S] (slice q's rows one contiguous region),
 * so a sliced sweep gathers from a region small enough to stay in the last-level
 * cache; s_in and s_out keep the node-major layout and tmp stays pure scratch.
 * slices >= 1 must divide U.  first_sliced == 0: the first sweep is one launch
 * over whole rows that writes every region, later sweeps run slice by slice
 * (s_out serves as second scratch buffer when steps >= 3); first_sliced != 0:
 * every sweep runs slice by slice, a slice's whole chain before the next slice
 * starts, through two regions of tmp.  steps <= 1 or slices == 1 run as
 * mjx_rollout_ell_rp_sliced.  The result is identical for every choice. */
int mjx_rollout_ell_rp_sm(const int32_t* adj, int64_t n, int d, int64_t words,
                          const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                          int steps, int slices, int first_sliced,
                          unsigned long long* counts, void* stream);
/* What slices = 0 runs (host only, no device call): *slices, *slice_major
 * (0: mjx_rollout_ell_rp_sliced's node-major slicing, 1: mjx_rollout_ell_rp_sm)
 * and *first_sliced.  One node-major slice when the state fits the cache, when
 * steps < 2, or when no slice count dividing U fits the cache budget. */
int mjx_rollout_ell_rp_plan(int64_t n, int d, int64_t words, int steps,
                            int* slices, int* slice_major, int* first_sliced);
int mjx_rollout_csr_np(const int64_t* row_ptr, const int32_t* col, int64_t n,
                       const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                       int steps, unsigned long long* counts, void* stream);
int mjx_rollout_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t words,
                       const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                       int steps, unsigned long long* counts, void* stream);

/* mjx_rollout_csr_rp with a node visiting order (int32 permutation of 0..n-1,
 * nullable): sorted by degree, the two nodes a wavefront holds share one trip
 * count.  Results do not depend on the order. */
int mjx_rollout_csr_rp_ordered(const int64_t* row_ptr, const int32_t* col, const int32_t* order, int64_t n,
                               int64_t words, const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                               int steps, unsigned long long* counts, void* stream);

/* Degree-class ELL: the notebook's own ER layout (nb:113-117 sums
 * s[N_nodes_pos[d]] for the nodes nodes_with_d_positions[d] of each degree
 * class; nb:359-361 builds them), replacing mjx_rollout_csr_rp(_ordered)
 * (`onestep_majority`, nb:113-117; `s_endstate`, nb:120-123).
 * classes: HOST int64 array of nclasses rows {i0, count, D, base}: positions
 * [i0, i0+count) of `order` hold the class's nodes, all of degree D
 * (0 <= D <= 255), and node order[i0+k]'s neighbours are cell[base+k*D ..
 * base+k*D+D); base is a multiple of 4; the counts sum to n.
 * mjx_class_ell_fill writes `cell` from CSR (setup); mjx_rollout_class_rp has
 * the contract of mjx_rollout_csr_rp.  Results do not depend on the layout. */
int mjx_class_ell_fill(const int64_t* row_ptr, const int32_t* col, const int32_t* order,
                       const int64_t* classes, int nclasses, int64_t n, int32_t* cell, void* stream);
int mjx_rollout_class_rp(const int32_t* order, const int32_t* cell, const int64_t* classes, int nclasses,
                         int64_t n, int64_t words, const uint64_t* s_in, uint64_t* s_out, uint64_t* tmp,
                         int steps, unsigned long long* counts, void* stream);
/* Measurement only (no reference counterpart): the class sweep's memory traffic
 * without the majority -- per position its D neighbour rows, its own row where D
 * is even, the rows' XOR written to s_out -- over the same arrays and grid, so
 * the bench can put the sweeps beside the random-row floor of the state. */
int mjx_gather_floor_class(const int32_t* order, const int32_t* cell, const int64_t* classes, int nclasses,
                           int64_t n, int64_t words, const uint64_t* s_in, uint64_t* s_out, void* stream);

/* per-replica count of +1 spins, ADDED into counts (m(s) = (2*count-n)/n) */
int mjx_popcount_np(const uint64_t* bits, int64_t n, unsigned long long* counts, void* stream);
int mjx_popcount_rp(const uint64_t* bits, int64_t n, int64_t words,
                    unsigned long long* counts, void* stream);

/* ---- run to the attractor (no reference counterpart) -------------------- */
/*
 * Synchronous majority dynamics with always-stay ties on an undirected graph
 * end in a fixed point or a 2-cycle (Goles & Olivos).  Definitions, for one
 * replica:
 *   trajectory  s(0) = s0, s(t+1) = onestep_majority(s(t));
 *   p = min{ t >= 0 : s(t+2) = s(t) }   (once it holds it holds for all later t);
 *   c = 1 if s(p+1) = s(p), else c = 2;
 *   with a sweep budget t_max a replica with p > t_max reports p = -1, c = 0;
 *   sum_att[r] = (sum s(p), sum s(p+1)): equal when c = 1; consensus means
 *   both equal n.
 *
 * mjx_sweep_track_ell_rp / mjx_sweep_track_csr_rp: one step of
 * mjx_rollout_ell_rp / mjx_rollout_csr_rp_ordered (s_out = onestep(s_in);
 * counts nullable, [64*words] added) plus tracking.  diff: uint64[2*words],
 * ORed into (caller zeroes it): bit r&63 of diff[r>>6] is set iff some node of
 * replica r has s_out != s_in; bit r&63 of diff[words + (r>>6)] iff some node
 * has s_out != s_prev.  s_prev is nullable: that half is then untouched.
 * s_out may be the same buffer as s_prev (the ping-pong case: every word is
 * read and then written by the one thread that owns it); s_out may not alias
 * s_in, nor s_prev s_in.  Padding replicas (bits 0 in every state, as
 * mjx_pack_rp and mjx_random_spins_rp write them) never set a flag.
 * Out of scope: the degree-class ELL layout, the node-packed layout and a
 * graph per replica (rep_graph).
 */
int mjx_sweep_track_ell_rp(const int32_t* adj, int64_t n, int d, int64_t words,
                           const uint64_t* s_in, const uint64_t* s_prev, uint64_t* s_out,
                           unsigned long long* counts, uint64_t* diff, void* stream);
int mjx_sweep_track_csr_rp(const int64_t* row_ptr, const int32_t* col, const int32_t* order, int64_t n,
                           int64_t words, const uint64_t* s_in, const uint64_t* s_prev, uint64_t* s_out,
                           unsigned long long* counts, uint64_t* diff, void* stream);
/* Bookkeeping after tracked sweep k >= 2 (which wrote s(k)): diff = that
 * sweep's flags, diff_prev = those of sweep k-1 (its first half is read),
 * cnt_km2 / cnt_km1 = the +1 counts of s(k-2) / s(k-1).  Every replica r < R
 * with p[r] == -1 whose "s(k) != s(k-2)" bit is clear gets p[r] = k-2, c[r] =
 * 2 if its "s(k-1) != s(k-2)" bit is set else 1, sum_att[2r], sum_att[2r+1] =
 * 2*cnt - n of s(k-2), s(k-1); *unsettled drops by the number settled.  The
 * caller starts with p = -1, c = 0, *unsettled = R. */
int mjx_attractor_record(int64_t n, int64_t R, int k, const uint64_t* diff, const uint64_t* diff_prev,
                         const unsigned long long* cnt_km2, const unsigned long long* cnt_km1,
                         int32_t* p, int32_t* c, int64_t* sum_att, unsigned long long* unsettled, void* stream);
/* Random starts, replica-packed bits[n*ceil(R/64)]: bit (v, r) is 1 iff
 * x < floor(prob[r] * 2^32) compared in 64 bits (prob: device double[R] in
 * [0, 1]; 1 gives all +1, 0 all -1), x = word r&3 of philox4x32_10(counter =
 * (v_lo, v_hi, r>>2, 0), key = (seed_lo, seed_hi)): a pure function of
 * (seed, v, r), whatever R is.  Padding replicas are 0. */
int mjx_random_spins_rp(int64_t n, int64_t R, uint64_t seed, const double* prob, uint64_t* bits, void* stream);

/* ---- simulated annealing (code/SA_RRG.py:44-92), R = 64*W replicas ------ */
/*
 * Per-replica state, all device arrays of length R unless noted.  Replica r
 * replays numpy's legacy global MT19937 after np.random.seed(seeds[r]):
 * binomial(1,.5,n) for s0 (code/SA_RRG.py:65), then per step
 * randint(0,n) (:73) and rand() (:76).
 */
typedef struct mjx_sa_state {
    uint32_t* mt;        /* [R*624] MT19937 words, replica-major: mt[r*624 + k] */
    int32_t*  mt_idx;    /* [R] next word index (624 = twist pending)        */
    double*   a;         /* [R] annealing weight a (code/SA_RRG.py:67,80)    */
    double*   b;         /* [R] annealing weight b (:68,81)                  */
    int64_t*  t;         /* [R] proposals made (:82)                         */
    int64_t*  sum_end;   /* [R] sum of s_endstate(s) over nodes (+-1 sum)    */
    int32_t*  done;      /* [R] 0 running, 1 consensus reached, 2 cap hit    */
    int32_t*  prop_i;    /* [R] scratch: proposed node                       */
    int8_t*   prop_s;    /* [R] scratch: spin of the proposed node before the flip */
    double*   prop_u;    /* [R] scratch: accept uniform                      */
    unsigned long long* cnt; /* [R] scratch: +1 count of the rolled-out proposal */
    /* optional per-step trace (NULL to disable); row k = step k of this call */
    int32_t*  tr_i;      /* [nsteps*R] proposed node (-1 if replica done)    */
    int8_t*   tr_acc;    /* [nsteps*R] 1 accepted, 0 rejected, -1 done       */
    int64_t*  tr_sum;    /* [nsteps*R] sum_end after the step               */
    double*   tr_dE;     /* [nsteps*R] delta_H (code/SA_RRG.py:74)          */
    int32_t*  tr_tie;    /* [R] count of |u - exp(-dE)| < 4 ulp near-ties    */
    /* optional proposal tape for mjx_sa_lightcone_steps (NULL / 0 to draw
     * inside the step kernel): the (i, u) of up to tape_cap steps of every
     * replica are drawn ahead by a wave per replica; replica-major: entry
     * (r, k) at r * tape_cap + k, k = step k of the chunk (the library may
     * split the buffer into two halves of tape_cap / 2 rows per replica) */
    int32_t*  tape_i;    /* [tape_cap*R] */
    double*   tape_u;    /* [tape_cap*R] */
    int64_t   tape_cap;
    /* distinct graphs (nullable = every replica on the one graph `adj`):
     * replica r runs on graph rep_graph[r] (device int32[R]) of a stack of
     * graphs with the same n and d, graph g's rows at adj + g*n*d (and at
     * adj_pad + g*n*4 for the padded d = 3 rows).  The reference draws a
     * fresh graph per replica (code/SA_RRG.py:58-62). */
    const int32_t* rep_graph;
    /* light-cone kernel selection, 0 = the library's choice (tests and tuning
     * set them; nothing is read from the environment) */
    int32_t   opt_split;   /* waves per 64-replica word column: 1, 2, 4, ..., 64 */
    int32_t   opt_spec_k;  /* speculative batch width: 8 or 16 */
    uint32_t  opt_flags;   /* MJX_SA_NO_SPEC | MJX_SA_NO_CONE2 | MJX_SA_LDS_* */
    /* nullable: the NON-parity proposal stream.  When set,
     * the tape of mjx_sa_lightcone_steps / _cone_steps / _rec_steps (tape_cap
     * > 0, required) is drawn by Philox-4x32-10 instead of the MT19937 replay:
     * the proposal of step t of replica r is philox4x32_10(counter (t_lo,
     * t_hi, 0, 0), key (k_lo, k_hi)) with k = philox_key[r]: i = the high 64
     * bits of (x0 | x1 << 32) * n, u = (x2 >> 5, x3 >> 6) as numpy's rand().
     * A pure function of (key, t): any chunking, any kernel, same run.  The
     * steps that draw inside the kernel (mjx_sa_steps, mjx_sa_lds_steps)
     * refuse it (MJX_EINVAL). */
    const uint64_t* philox_key;   /* [R] */
    /* library-kept: 1 while the neighbour words of a d = 3, p+c-1 = 2 record
     * array (mjx_sa_rec_*) are current.  mjx_sa_rec_pack writes them; the
     * speculative steps keep them; any other light-cone kernel leaves them
     * stale and sets 0; the next speculative call rebuilds them first.  Start
     * at 0 (a zeroed struct). */
    int32_t   rec_nb;
} mjx_sa_state;

#define MJX_SA_NO_SPEC   1u   /* no speculative batches (k_sa_spec) */
#define MJX_SA_NO_CONE2  2u   /* no one-round-trip step (k_sa_cone2) */
#define MJX_SA_LDS_SERIAL 4u  /* LDS layout: the list-based step (k_sa_lds), not the lane-held one */
#define MJX_SA_LDS_SINGLE 8u  /* LDS layout: one proposal per step (k_sa_lds_fast), not two (k_sa_lds_pair) */
#define MJX_SA_LDS_PAIR  16u  /* LDS layout at p+c-1 = 1: two proposals per step, not eight (k_sa_lds_multi) */
#define MJX_SA_LDS_WAVE  32u  /* LDS layout at p+c-1 >= 2: one wave per replica (k_sa_lds_pair), not the whole
                                 CU (k_sa_lds_wg: opt_split = 4, 8 or 16 waves, one proposal each) */
#define MJX_SA_LDS_CU    64u  /* LDS layout at p+c-1 = 2, 3, d = 3, 4: the whole CU level by level (k_sa_lds_cu:
                                 15 proposals a round, each level's candidates packed over the waves; 8 waves,
                                 16 with opt_split = 16).  The default there where it fits and no other
                                 option is given; opt_split = 4, 8 or 16 alone select k_sa_lds_wg */

/* Seed replica r with seeds[r] (device uint32[R]), draw s0 into the
 * replica-packed spins s[n*W], set a=a0, b=b0, t=0, done=0, and
 * sum_end = sum(s_endstate(s0)) using tmp1/tmp2 ([n*W] each); with
 * st->rep_graph each replica's rollout runs on its own graph. */
int mjx_sa_init(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R,
                const uint32_t* seeds, double a0, double b0,
                uint64_t* s, uint64_t* tmp1, uint64_t* tmp2,
                mjx_sa_state* st, void* stream);

/* As mjx_sa_init, but replica r continues a given MT19937 stream instead of
 * seeding one: mt_in [R*624] words and idx_in [R] next-word indices (device),
 * e.g. the state another replica ended in.  This is how the reference's
 * N_stat replicas share numpy's ONE global stream back to back
 * (code/SA_RRG.py:58-65: replica k+1's s0 draws follow replica k's last rand()). */
int mjx_sa_init_mt(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R,
                   const uint32_t* mt_in, const int32_t* idx_in, double a0, double b0,
                   uint64_t* s, uint64_t* tmp1, uint64_t* tmp2,
                   mjx_sa_state* st, void* stream);

/* Advance every running replica by `nsteps` proposals (code/SA_RRG.py:72-85),
 * full rollout of each proposal.  par_a/par_b: annealing factors (:49-50);
 * a_cap = 4.5*n, b_cap = 5*n (:80-81); t_cap = 2*n**3 (:84). */
int mjx_sa_steps(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R,
                 uint64_t* s, uint64_t* tmp1, uint64_t* tmp2,
                 mjx_sa_state* st, int64_t nsteps,
                 double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap,
                 void* stream);

/* Light-cone SA: the same proposals, accept decisions and
 * outputs as mjx_sa_steps, but each proposal is evaluated only inside the ball
 * of radius p+c-1 around the flipped node, from cached rollout levels.
 * levels: host array of T = p+c-1 device pointers, levels[t-1] = onestep^t(s)
 * (n*W words each), kept consistent by the kernel as flips are accepted.
 * mjx_sa_lightcone_prepare fills them from s (call after mjx_sa_init).
 * Supported: 1 <= T <= 6, d <= 16 and mjx_sa_lightcone_lds(d,p,c) <= 150 KiB
 * (bytes of LDS per 64 replicas; -1 if unsupported).  The step kernel runs
 * several waves per 64-replica word column when the column count is small
 * (st->opt_split overrides the choice).  rep_graph (nullable): as in
 * mjx_sa_state, for the levels of replicas on distinct graphs. */
int64_t mjx_sa_lightcone_lds(int d, int p, int c);
int mjx_sa_lightcone_prepare(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R,
                             const int32_t* rep_graph, const uint64_t* s, uint64_t* const* levels,
                             void* stream);
int mjx_sa_lightcone_steps(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R,
                           uint64_t* s, uint64_t* const* levels, mjx_sa_state* st, int64_t nsteps,
                           double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap,
                           void* stream);

/* Cone layout of the cached levels: the T+1 words (s, onestep(s), ...,
 * onestep^T(s)) of one (node, word column) side by side, padded to
 * LV = mjx_sa_cone_words(p,c) words (2, 4 or 8; -1 if unsupported), word
 * column major: cone[(w*n + v)*LV + t] = level t, word w of node v (n*W*LV
 * words).  A
 * proposal reads several levels of the same nodes; here they share one
 * memory sector.  mjx_sa_cone_pack builds the cone from s and the separate
 * levels (after mjx_sa_lightcone_prepare); mjx_sa_cone_steps is
 * mjx_sa_lightcone_steps on the cone (same proposals, accepts and outputs),
 * mirroring every accepted level-0 flip into s so s stays the configuration;
 * mjx_sa_cone_unpack writes the cone back to s and the separate levels.
 * adj_pad (optional, d = 3): the adjacency with rows padded to 4 int32
 * (n*4, 16-B aligned); with it, p+c-1 = 2 and a proposal tape, every proposal
 * costs one memory round trip (rows fetched down the tape ahead of time). */
int mjx_sa_cone_words(int p, int c);
int mjx_sa_cone_pack(int64_t n, int p, int c, int64_t R, const uint64_t* s,
                     uint64_t* const* levels, uint64_t* cone, void* stream);
int mjx_sa_cone_unpack(int64_t n, int p, int c, int64_t R, const uint64_t* cone,
                       uint64_t* s, uint64_t* const* levels, void* stream);
int mjx_sa_cone_steps(const int32_t* adj, const int32_t* adj_pad, int64_t n, int d, int p, int c, int64_t R,
                      uint64_t* s, uint64_t* cone, mjx_sa_state* st, int64_t nsteps,
                      double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap,
                      void* stream);

/* Record layout: the cone with each (node, word column) sector preceded by the
 * node's adjacency row (int32 x4, zero padded): rec[(w*n + v)*LV + e], words
 * 0..1 = the row, word 2 + t = level t, LV = mjx_sa_rec_words(d,p,c) (4 or 8;
 * -1 if unsupported: d <= 4, p+c-1 <= 5).  The speculative step then fetches a
 * ball node's row and levels in one line.  At d = 3, p+c-1 = 2 the record's
 * spare 28 bytes (the row's pad int, words 5..7) hold its neighbours' level-1
 * bits, 3 per replica (st->rec_nb).  One graph shared by every replica
 * (st->rep_graph must be NULL).  Same proposals, accepts and outputs as every
 * other layout. */
int mjx_sa_rec_words(int d, int p, int c);
/* sizeof(mjx_sa_state) as the library was built (a binding checks its mirror) */
int mjx_sa_state_bytes(void);
int mjx_sa_rec_pack(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R, const uint64_t* s,
                    uint64_t* const* levels, uint64_t* rec, void* stream);
int mjx_sa_rec_unpack(int64_t n, int d, int p, int c, int64_t R, const uint64_t* rec, uint64_t* s,
                      uint64_t* const* levels, void* stream);
int mjx_sa_rec_steps(const int32_t* adj, const int32_t* adj_pad, int64_t n, int d, int p, int c, int64_t R,
                     uint64_t* s, uint64_t* rec, mjx_sa_state* st, int64_t nsteps,
                     double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap,
                     void* stream);

/* LDS-resident light-cone SA (small graphs, the reference's own sizes: n = 1e4,
 * d = 4, code/SA_RRG.py:44-52): a workgroup per replica keeps its graph (uint16
 * rows), the rollout levels onestep^t(s) (t = 0..p+c-1, bit arrays) and its
 * MT19937 state in LDS for the whole call; levels are rebuilt from s at the
 * start of every call, the changed configuration bits XORed back into s and
 * the stream state written back at its end (exactly numpy's position: nothing
 * is drawn ahead).  Same proposals, accepts and outputs as mjx_sa_steps;
 * honours st->rep_graph and the trace pointers; no tape, no level arrays.
 * mjx_sa_lds_bytes: LDS bytes per replica, -1 if (n, d, p, c) does not fit
 * (n <= 65535, d <= 16, 1 <= p+c-1 <= 6, <= 160 KiB). */
int64_t mjx_sa_lds_bytes(int64_t n, int d, int p, int c);
/* LDS bytes per replica of the kernel mjx_sa_lds_steps selects for these
 * kernel options (opt_flags, opt_split), its threads per workgroup in
 * *threads (64, or 64 per wave of the whole-CU kernel); -1 if it does not fit. */
int64_t mjx_sa_lds_plan(int64_t n, int d, int p, int c, uint32_t flags, int split, int* threads);

/* Host-only self-check of the per-device memo tables (CU counts, occupancy,
 * dynamic-LDS opt-ins are kept per device id, not per process): no HIP call,
 * runs without a GPU; 0 = pass, else the number of the failed check. */
int mjx_selftest_devmemo(void);
int mjx_sa_lds_steps(const int32_t* adj, int64_t n, int d, int p, int c, int64_t R, uint64_t* s,
                     mjx_sa_state* st, int64_t nsteps, double par_a, double par_b, double a_cap, double b_cap,
                     int64_t t_cap, void* stream);

/* ---- simulated annealing on irregular graphs (CSR) ----------------------- */
/* The loop of code/SA_RRG.py:65-85 on a graph given as CSR (row_ptr int64
 * [n+1], col int32 [nnz]; one graph for all replicas), scored with the
 * notebook's ER end state (nb:113-123: sign(2S+s), a degree-0 node keeps its
 * spin).  Replica r replays np.random.seed(seeds[r]) exactly as on regular
 * graphs; the schedule constants are the caller's (schedule of n = the node
 * count of the graph as passed).  Row entries count with multiplicity (a
 * self-loop or a doubled edge contributes as often as it is listed).  On the
 * CSR of a d-regular neighbour array every call is bit-identical to its
 * mjx_sa_* counterpart.
 *
 * PRECONDITION of the light-cone calls: the adjacency is symmetric as a
 * multiset of directed entries (v appears in row(u) as often as u in row(v)).
 * The light cone finds the nodes that read a changed node in that node's own
 * row.  The full-rollout calls (init, steps) do not need it.
 * st->rep_graph and (steps) st->philox_key are refused with MJX_EINVAL. */
int mjx_sa_csr_init(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                    const uint32_t* seeds, double a0, double b0, uint64_t* s, uint64_t* tmp1, uint64_t* tmp2,
                    mjx_sa_state* st, void* stream);
int mjx_sa_csr_init_mt(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                       const uint32_t* mt_in, const int32_t* idx_in, double a0, double b0, uint64_t* s,
                       uint64_t* tmp1, uint64_t* tmp2, mjx_sa_state* st, void* stream);
/* Full-rollout step (the exact slow path and in-library cross-check):
 * proposal, mjx_rollout_csr_rp with the fused +1 count, Metropolis test. */
int mjx_sa_csr_steps(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                     uint64_t* s, uint64_t* tmp1, uint64_t* tmp2, mjx_sa_state* st, int64_t nsteps,
                     double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap, void* stream);
/* Ball bound: B_0(v) = 1, B_t(v) = 1 + sum_{k in row(v)} B_{t-1}(k) (walks of
 * length <= t from v), saturating; bound_out[t] = min(n, max_v B_t(v)), t =
 * 0..T (HOST array).  cap_t bounds the candidate set and the changed set of
 * level t of any proposal.  work: mjx_sa_csr_ball_work_bytes(n) bytes of device
 * scratch.  Setup call: synchronises `stream`.  0 <= T <= 6. */
int64_t mjx_sa_csr_ball_work_bytes(int64_t n);
int mjx_sa_csr_ball_bound(const int64_t* row_ptr, const int32_t* col, int64_t n, int T, void* work,
                          int64_t* bound_out, void* stream);
/* Light-cone step on CSR.  Per replica T+2 lists (changed nodes of levels
 * 0..T, candidates); the first lds_entries entries of each list per lane live
 * in LDS (0 = the library's choice, 32), the rest in the caller's spill area.
 * caps: HOST int64 [T+1] from mjx_sa_csr_ball_bound (any graph within its caps
 * is evaluated exactly; a replica whose lists outgrow wrong caps stops with
 * done = 3, nothing is written out of bounds).
 * _lds: LDS bytes of a workgroup (-1: T or lds_entries out of range, more than
 * 150 KiB); _scratch_bytes: bytes of spill area for R replicas (0 when every
 * list fits LDS; -1 on bad arguments). */
int64_t mjx_sa_csr_lightcone_lds(int T, int lds_entries);
int64_t mjx_sa_csr_lightcone_scratch_bytes(int64_t R, int T, const int64_t* caps, int lds_entries);
/* levels[t-1] = onestep^t(s), t = 1..T = p+c-1 (mjx_rollout_csr_rp) */
int mjx_sa_csr_lightcone_prepare(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                                 const uint64_t* s, uint64_t* const* levels, void* stream);
/* One persistent launch over nsteps proposals, a wave per word column of 64
 * replicas (st->opt_split waves per column when set, as mjx_sa_lightcone_steps);
 * proposals are drawn in the step (no tape: the streams stand exactly where
 * numpy's would); honours the trace pointers and tr_tie; s and levels are kept
 * current.  MJX_EINVAL for st->rep_graph, st->philox_key, T < 1, T > 6 or
 * spill_bytes below _scratch_bytes.  No allocation, no host synchronisation. */
int mjx_sa_csr_lightcone_steps(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t R,
                               uint64_t* s, uint64_t* const* levels, mjx_sa_state* st, int64_t nsteps,
                               double par_a, double par_b, double a_cap, double b_cap, int64_t t_cap,
                               const int64_t* caps, int lds_entries, void* spill, int64_t spill_bytes,
                               void* stream);
/* Diagnostic: out2[0] = proposals evaluated by mjx_sa_csr_lightcone_steps on
 * the current device since the last reset, out2[1] = those with a list longer
 * than its LDS part (the spill rate's numerator).  Synchronises the device. */
int mjx_sa_csr_lightcone_stats(unsigned long long* out2, int reset);

/* ---- history-passing reinforcement on d-regular graphs ------------------ */
/*
 * Message arrays use the reference's layout (code/HPR_pytorch_RRG.py:277-285, 46-61):
 * chi[2E][4^T], T = p+c, E = n*d/2; row r < E is G.edges[r] = (u,v) as the
 * message u->v, row r+E is v->u; column of (x_a, x_b) is idx(x_a)*2^T + idx(x_b)
 * with idx(x) = sum_k [x_k = -1] 2^(T-1-k).  Node-major plan arrays, all [n*d]:
 *   nbr[a*d+m]     = m-th neighbour k_m of a
 *   in_row[a*d+m]  = row of the message k_m -> a
 *   out_row[a*d+m] = row of the message a -> k_m   (the reference's N_edges_pos)
 * biases[n][2]: column 0 = bias of spin +1.  dtype MJX_F32 or MJX_F64 for chi,
 * biases, marginals and zwork.
 */
/* HPr_dp (code/HPR_pytorch_RRG.py:183-218): chi_out = damp*chi_new/rowsum +
 * (1-damp)*chi_in, where chi_new carries the reinforced incoming messages
 * (new_biases_chi, :128-133) and the trajectory factor A (:14-39).
 * w_plus / w_minus = exp(-lmbd_in*x_a[0]/n) for x_a[0] = +1 / -1.
 * Supported: 2 <= p+c <= 4, 2 <= d <= 6 (MJX_ERANGE otherwise).
 * chi_in may not alias chi_out. */
int mjx_hpr_update(int dtype, const void* chi_in, void* chi_out, const void* biases,
                   const int32_t* nbr, const int32_t* in_row, const int32_t* out_row,
                   int64_t n, int d, int p, int c, int attr_value,
                   double w_plus, double w_minus, double damp, void* stream);
/* marginals_comp (code/HPR_pytorch_RRG.py:147-167): marg[n][2] (column 0 = +1).
 * zwork: 4E elements of dtype (per-row normalised Z+, Z-). */
int mjx_hpr_marginals(int dtype, const void* chi, const int32_t* out_row, int64_t n, int d,
                      int p, int c, double eps, void* zwork, void* marg, void* stream);
/* new_biases_i (code/HPR_pytorch_RRG.py:137-145) with the uniforms u[n] (float64) the
 * reference draws by torch.rand(n); thresh = 1-(1+t)^(-gamma).  Updates biases in
 * place and writes s[n] = +-1 (int32, nullable). */
int mjx_hpr_new_biases(int dtype, void* biases, const void* marg, const double* u, double thresh,
                       double pie, int64_t n, int32_t* s, void* stream);
/* The same with the comparison u_i < thresh made by the caller: refresh[n] (uint8,
 * nonzero = refresh node i's biases). */
int mjx_hpr_new_biases_mask(int dtype, void* biases, const void* marg, const uint8_t* refresh, double pie,
                            int64_t n, int32_t* s, void* stream);

/* One node step of the HPR main loop in one launch (code/HPR_pytorch_RRG.py:
 * 147-167 node part, 137-145, and the bit packing of s for :352): node
 * marginals from the edge Z sums in zwork (mjx_hpr_marginals_q with marg =
 * NULL computes only those), the bias refresh where refresh[v] (as
 * mjx_hpr_new_biases_mask), s[v] = +-1 and its node-packed bits (as
 * mjx_pack_np).  Replaces mjx_hpr_marginals' node part + new_biases_mask +
 * pack_np; same values. */
int mjx_hpr_node_step(int dtype, const void* zwork, const int32_t* out_row, int64_t n, int d, void* marg,
                      void* biases, const uint8_t* refresh, double pie, int32_t* s, uint64_t* bits, void* stream);
/* The reference's torch.rand(n) per iteration (torch's CPU generator, :142) on the
 * device: state[624] (uint32) and left_next[2] = the CPU engine's `left`, `next`
 * (its get_state() fields); k iterations of n float64 uniforms u = ((y_hi<<32 |
 * y_lo) & (2^53-1)) * 2^-53 from consecutive outputs, compared with thresh[j]
 * (device float64) into mask[j*n + i] (uint8).  state/left_next are left where the
 * CPU generator would be after the same draws.  One workgroup; run it on a
 * stream of its own beside the iterations that consume the masks. */
int mjx_hpr_refresh_masks(uint32_t* state, int32_t* left_next, int64_t n, int k, const double* thresh,
                          uint8_t* mask, void* stream);
/* The same draws by G workgroups at once (MT19937 jump-ahead, csrc/mjx_mtjump.hip):
 * the batch's 2nk words are split into chunks of L words (a multiple of 624), chunk
 * j's workgroup jumps the batch-start state ahead by jL-1 words with the polynomial
 * z^(jL-1) mod P (P = the characteristic polynomial of MT19937's state map).
 * mjx_mt_jump_geometry: L and the number of chunks actually used for (n, k, G);
 * mjx_mt_jump_table_words / mjx_mt_jump_table: the (chunks-1) x 312 uint64 table
 * of those polynomials, computed on the HOST (setup, once per (n, k, G));
 * mjx_hpr_refresh_masks_jump: reads state_in/ln_in (the engine at the batch start),
 * writes state_out/ln_out (after the batch; must not alias the inputs), the masks
 * as mjx_hpr_refresh_masks; `table` is the device copy. */
int mjx_mt_jump_geometry(int64_t n, int k, int G, int64_t* L, int* G_used);
int64_t mjx_mt_jump_table_words(int64_t n, int k, int G);
int mjx_mt_jump_table(int64_t n, int k, int G, uint64_t* table);
int mjx_hpr_refresh_masks_jump(const uint32_t* state_in, const int32_t* ln_in, uint32_t* state_out,
                               int32_t* ln_out, int64_t n, int k, int G, const uint64_t* table,
                               const double* thresh, uint8_t* mask, void* stream);
/* mjx_hpr_refresh_masks_jump for `instances` independent streams at once (HPR on
 * a union of graphs, one torch CPU generator per instance): instance g's engine
 * is state_in + 624 g and ln_in + 2 g (likewise the outputs), continued by
 * `chunks` workgroups as above; each instance may stand anywhere in its 624-word
 * block.  thresh[k] is shared (the instances walk t in lockstep), and so is
 * `table`, which is mjx_mt_jump_table(n, k, chunks).  Row `it` of the mask holds
 * every instance's decisions: mask[(it * instances + g) * n + i]. */
int mjx_hpr_refresh_masks_jump_batch(const uint32_t* state_in, const int32_t* ln_in, uint32_t* state_out,
                                     int32_t* ln_out, int64_t n, int k, int chunks, int64_t instances,
                                     const uint64_t* table, const double* thresh, uint8_t* mask, void* stream);
/* The consensus test and stop of the HPR loop (code/HPR_pytorch_RRG.py:352-356)
 * for the G instances of a union graph, on the device.  bits: the node-packed
 * end state of the rollout (G*n bits, instance g = bits [g*n, (g+1)*n)), s[G*n]
 * the trial configuration, t = (*t_base, device, nullable = 0) + t_add the
 * iteration reached.  counts[g] = the +1 bits of instance g's range.  With o =
 * inst[g] (nullable: o = g), an instance with done[o] == 0 stops if t > TT
 * (done[o] = 2), else if counts[g] == n (done[o] = 1): t_stop[o] = t,
 * conf[o*n .. o*n+n) = its slice of s, *live drops by one.  An instance with
 * done[o] != 0 is never written again. */
int mjx_hpr_batch_record(const uint64_t* bits, const int32_t* s, int64_t n, int64_t G, const int32_t* inst,
                         const int64_t* t_base, int64_t t_add, int64_t TT, unsigned long long* counts,
                         int32_t* done, int64_t* t_stop, int32_t* conf, unsigned long long* live, void* stream);
/* The edge half of marginals_comp (code/HPR_pytorch_RRG.py:150-161) alone:
 * zwork[4E] = per-row normalised (Z+ [2E], Z- [2E]) of every directed row. */
int mjx_hpr_edge_z(int dtype, const void* chi, int64_t E, int p, int c, double eps, void* zwork,
                   void* stream);
/* Node-indexed bias pairs for mjx_hpr_update from the reference's own bias arrays:
 * out[2v+k] = src[idx[v]*stride + k*half], k = 0, 1.  From biases_chi
 * (new_biases_chi, code/HPR_pytorch_RRG.py:128-133): stride = 4^T, half = 4^T/2 and
 * idx[v] = a row whose source node is v; from biases_i: stride 2, half 1. */
int mjx_hpr_node_biases(int dtype, const void* src, const int64_t* idx, int64_t stride, int64_t half,
                        int64_t n, void* out, void* stream);
/* The decay-split layout of the HPR loop state.  HPr_dp writes nothing into the
 * entries of a row whose sender trajectory is invalid (x_s[T-1] != attr_value):
 * they are only damped, chi_t = (1-damp)^t chi_0 (code/HPR_pytorch_RRG.py:215).
 * The loop state keeps each row as quadrants VV | VI | IV | II of (2^(T-1))^2
 * entries (first letter: sender valid/invalid, second: receiver), entry
 * (x_s, x_r) at quad*4^(T-1) + (x_s>>1)*2^(T-1) + (x_r>>1); the IV and II quadrants
 * hold chi_0 undecayed and are read with the scale (1-damp)^t from device
 * memory, so an update reads and writes only the first half of its own rows and
 * the VV and IV quadrants of its incoming rows.
 * mjx_hpr_q_supported: 1 if mjx_hpr_update_q runs this (dtype, d, p, c)
 * (MJX_F32, p+c = 4, 2 <= d <= 4).  mjx_hpr_qlayout: to_q = 1: dst = src
 * (reference layout) permuted; to_q = 0: dst = src (decay-split) in the reference
 * layout with the invalid-sender entries times scale.  mjx_hpr_update_q: HPr_dp on
 * the decay-split layout, *scale_in = chi_in's scale (dtype); chi_out's IV and II
 * quadrants are not written (they must already hold chi_0).  mjx_hpr_marginals_q:
 * marginals_comp of a decay-split chi with scale *scale (marg = NULL: only the
 * edge Z sums into zwork, for mjx_hpr_node_step). */
int mjx_hpr_q_supported(int dtype, int d, int p, int c);
int mjx_hpr_qlayout(int dtype, const void* src, void* dst, int64_t rows, int p, int c, int attr_value, int to_q,
                    double scale, void* stream);
int mjx_hpr_update_q(int dtype, const void* chi_in, void* chi_out, const void* biases, const int32_t* nbr,
                     const int32_t* in_row, const int32_t* out_row, int64_t n, int d, int p, int c,
                     int attr_value, double w_plus, double w_minus, double damp, const void* scale_in,
                     void* stream);
int mjx_hpr_marginals_q(int dtype, const void* chi, const int32_t* out_row, int64_t n, int d, int p, int c,
                        double eps, const void* scale, const void* ii, void* zwork, void* marg, void* stream);
/* ii[4E] (dtype): per edge the four sums of its II x II products (by x_u[0] = +1/-1,
 * by x_v[0] = +1/-1), which never change: computed once from the loop state's
 * chi_0 quadrants; mjx_hpr_marginals_q then skips reading the II quadrants
 * (ii may be NULL: everything is read). */
int mjx_hpr_q_ii(int dtype, const void* chi, int64_t E, int p, int c, void* ii, void* stream);

/* ---- HPR on Erdos-Renyi graphs (the "general (ER)" HPR of code/README.md:1) -
 * HPr_dp with the degree taken per message: rows of degree class D (the
 * message a->b with deg(a) = D+1, rows[m] of them) read their D incoming rows
 * inc[m*D + j] (messages k_j -> a, k_j != b) whose senders are inc_src[m*D + j],
 * with the reinforced messages bias_k(x_k[0]) chi^{k->a} and the trajectory
 * factor of d-1 = D (code/HPR_pytorch_RRG.py:14-39,128-133,183-218); same row,
 * column and bias layouts as mjx_hpr_update.  Jacobi: every class reads chi_in
 * and writes its rows of chi_out.  w_plus/w_minus = exp(-lmbd*x_a[0]/n);
 * 2 <= p+c <= 4, any D <= 255.  A class whose count table (2^(T-1)*(D+1)^T
 * elements per message, double for either dtype) does not fit the 160 KiB LDS keeps it in `scratch`:
 * mjx_hpr_er_scratch_bytes(dtype, D, p, c) per message in flight (0: LDS
 * suffices, -1: unsupported); the call then runs ceil(m / (scratch_bytes /
 * that)) launches (MJX_ERANGE if scratch holds not even one table). */
int64_t mjx_hpr_er_scratch_bytes(int dtype, int D, int p, int c);
int mjx_hpr_er_update_class(int dtype, const void* chi_in, void* chi_out, const void* biases,
                            const int32_t* rows, const int32_t* inc, const int32_t* inc_src, int64_t m,
                            int D, int p, int c, int attr_value, double w_plus, double w_minus,
                            double damp, void* scratch, int64_t scratch_bytes, void* stream);
/* node marginals over CSR out-rows (row of i->k for every neighbour k of i):
 * marg[i] = normalised (prod Z+, prod Z-) of zwork from mjx_hpr_edge_z. */
int mjx_hpr_node_marg_csr(int dtype, const void* zwork, int64_t E, const int64_t* out_ptr,
                          const int32_t* out_rows, int64_t n, void* marg, void* stream);

/* ---- one giant graph partitioned by node range -- */
/* One synchronous sweep of the rows [row_lo, row_hi) of a node-packed state.
 * adj holds those rows only: adj[(v - row_lo)*d + k].  s_in / s_out are the
 * full ceil(n/64)-word states (s_in read anywhere, s_out written only in words
 * [row_lo/64, ceil(row_hi/64))).  row_lo must be a multiple of 64 and row_hi a
 * multiple of 64 or n.  counts (nullable): +1 spins among the written nodes,
 * added.  Replaces onestep_majority (code/SA_RRG.py:18-20) on one rank's rows. */
int mjx_sweep_ell_np_range(const int32_t* adj, int64_t n, int d, int64_t row_lo, int64_t row_hi,
                           const uint64_t* s_in, uint64_t* s_out, unsigned long long* counts, void* stream);

/* Source-binned (propagation-blocking) sweep (one replica, huge n; config C5).
 * Same result as mjx_sweep_ell_np_range (code/SA_RRG.py:18-20 on the rows
 * [row_lo, row_hi)); replaces its one-random-cache-line-per-slot gather.  A
 * static plan bins the (row_hi-row_lo)*d (destination, source) slots by source
 * block (1M nodes, staged in LDS) and destination tile (64K nodes, LDS byte
 * counters); a sweep is two streaming kernels (messages, then counts + rule).
 * mjx_binned_plan_shape fills sizes[6] = {src_lo_len (the phase-1 stream),
 * src_hi_len (0: src_hi is unused and may be NULL), off_len (uint16 elements
 * each), index_len (int64 elements), msg_words (uint64 per-sweep message
 * bits), work_bytes (device scratch for mjx_binned_build)}.
 * Limits: n <= 2^31-1, d <= 16; row_lo a multiple of 64, row_hi too unless
 * row_hi == n.  adj holds the rows' ELL entries (global node ids).  */
int mjx_binned_plan_shape(int64_t n, int d, int64_t row_lo, int64_t row_hi, int64_t* sizes);
int mjx_binned_build(const int32_t* adj, int64_t n, int d, int64_t row_lo, int64_t row_hi, uint16_t* src_lo,
                     uint16_t* src_hi, uint16_t* off, long long* index, void* work, int64_t work_bytes, void* stream);
/* apply_form: 0 = the library's choice, 1 = flat tile stream (K <= 960 source
 * blocks, MJX_ERANGE beyond), 2 = per-segment form. */
int mjx_sweep_binned(const uint16_t* src_lo, const uint16_t* src_hi, const uint16_t* off, const long long* index,
                     int64_t n, int d,
                     int64_t row_lo, int64_t row_hi, const uint64_t* s_in, uint64_t* msg, uint64_t* s_out,
                     unsigned long long* counts, int apply_form, void* stream);

/* Device Erdos-Renyi G(n, p) into CSR, replacing
 * nx.erdos_renyi_graph + isolate removal + relabelling of
 * code/ER_BDCM_entropy.ipynb (cell 'ER graph', nb:278-291) with
 * distributional parity: each pair i < j is an edge with probability p
 * (geometric skipping per row, counter-based uniforms of (seed, row, k)).
 * Rows are sorted; the result depends on (n, p, seed) only.  With
 * drop_isolated the degree-0 nodes are removed and the rest relabelled in
 * increasing order (nb:283-291).  row_ptr: int64[n+1] (the first *n_out + 1
 * entries are written), col: int32[col_cap]; *n_out = rows kept, *nnz_out =
 * 2 * edges.  If col_cap < *nnz_out the call returns MJX_ERANGE after setting
 * both (retry with a larger col).  work: mjx_er_work_bytes(n) bytes of device
 * scratch.  Setup call: synchronises `stream`.  n <= 2^31 - 2, 0 <= p < 1.  */
int64_t mjx_er_work_bytes(int64_t n);
int mjx_er_generate(int64_t n, double p, uint64_t seed, int drop_isolated, long long* row_ptr, int32_t* col,
                    int64_t col_cap, int64_t* n_out, int64_t* nnz_out, void* work, int64_t work_bytes, void* stream);

/* ---- device graph generation ----------------------- */
/* Random simple d-regular graph (configuration model through a keyed
 * pseudorandom stub permutation, then deterministic double-edge switches that
 * remove self-loops and multi-edges), replacing nx.random_regular_graph
 * (code/SA_RRG.py:59) with distributional parity.  Writes the ELL rows
 * [row_lo, row_hi) into adj[(row_hi-row_lo)*d]; every rank that calls it with
 * the same (n, d, seed) gets rows of the same graph.  work: device scratch of
 * work_words >= 3 uint64 (defect list; 1 + 2*65536 is ample).  This is a setup
 * call: it synchronises `stream` to run the repair on the host.  n_switches
 * (host, nullable) receives the number of switches made.  d <= 16. */
int mjx_rrg_generate(int64_t n, int d, uint64_t seed, int64_t row_lo, int64_t row_hi, int32_t* adj,
                     uint64_t* work, int64_t work_words, int64_t* n_switches, void* stream);
/* Host-only: partner stub of `stub` in the unrepaired pairing (-1 on bad input). */
int64_t mjx_rrg_partner_host(int64_t n, int d, uint64_t seed, int64_t stub);
/* Checks a full ELL adjacency: counts[0] += self-loops, counts[1] += entries
 * repeated in their row, counts[2] += entries whose reverse multiplicity
 * differs or that are out of range. */
int mjx_graph_check_ell(const int32_t* adj, int64_t n, int d, unsigned long long* counts, void* stream);

/* ---- BDCM on Erdos-Renyi graphs (code/ER_BDCM_entropy.ipynb), float64 ---- */
/*
 * chi[2E][4^T] in the notebook's layout (nb:150-154, 303-314): row r < E is
 * G.edges[r] = (i, j) as the message i -> j, row r + E is j -> i; column of
 * (x_i, x_j) = idx(x_i)*2^T + idx(x_j), idx(x) = sum_t [x_t = +1] 2^(T-1-t).
 * T = p + c <= 4.  An "edge class" is the set of messages a -> b with
 * deg(a) - 1 = D (nb:312-318): rows[m] are their chi rows, inc[m*D + k] the
 * rows of the D incoming messages k -> a (the notebook's N_edges_pos_dm1).
 * Any D <= 255: the count table of an item (2^(T-1)*(D+1)^T doubles) lives in
 * LDS when mjx_bdcm_lds_bytes(D, p, c) <= 160 KiB, else in the caller's
 * `scratch` slab, mjx_bdcm_scratch_bytes(D, p, c) per item in flight (0: LDS
 * suffices, -1: unsupported); the call then runs ceil(m / (scratch_bytes /
 * that)) launches (MJX_ERANGE if the slab holds not even one table).
 */
int64_t mjx_bdcm_lds_bytes(int D, int p, int c);
int64_t mjx_bdcm_scratch_bytes(int D, int p, int c);
/* One class of BDCM_ER (nb:150-196): new rows = damp*normalize(max(chi2, eps))
 * + (1-damp)*old, written to upd[m*4^T] and then committed into chi (the class
 * reads chi before any of its own rows change: Jacobi within a class,
 * Gauss-Seidel across classes when called in ascending D).  damp >= 1 assigns
 * normalize(chi2): with D = 0 that is the leaf reset of nb:404-417.
 * delta_bits (nullable): atomic max of |new - old| as IEEE bits (a NaN wins).
 * gate (nullable): when *gate != 0 on the device the launches do nothing (the
 * stop flag of a captured convergence loop, ctl + 1 below).
 * w_dev (nullable): two doubles {exp(-lmbd), exp(lmbd)} read on the device in
 * place of the lmbd argument, so one captured loop serves every lambda. */
int mjx_bdcm_update_class(double* chi, const int32_t* rows, const int32_t* inc, int64_t m, int D, int p, int c,
                          int attr_value, double lmbd, double damp, double eps, double* upd,
                          unsigned long long* delta_bits, const long long* gate, const double* w_dev, void* scratch,
                          int64_t scratch_bytes, void* stream);
/* The notebook's convergence loop on the device (nb:422-431: while delta > eps,
 * t += 1, stop at T_max), for capture in a hipGraph with one host read per
 * batch.  ctl[4] int64: [0] delta bits of the running sweep (pass ctl as
 * delta_bits), [1] stop flag (pass ctl + 1 as gate), [2] sweeps done t,
 * [3] delta bits of the last completed sweep.  begin: if not stopped, ctl[0] = 0;
 * end: if not stopped, t += 1, ctl[3] = ctl[0], stop when !(delta > eps) or
 * t >= t_max.  Zero ctl before the loop. */
int mjx_bdcm_iter_begin(long long* ctl, void* stream);
int mjx_bdcm_iter_end(long long* ctl, double eps, int64_t t_max, void* stream);
/* Zi_ER for the m nodes of degree D (nb:211-276): zi[nodes[k]] = max(Zi, eps);
 * inc[k*D + j] = row of the message from the j-th neighbour into the node. */
int mjx_bdcm_node_z(const double* chi, const int32_t* nodes, const int32_t* inc, int64_t m, int D, int p, int c,
                    int attr_value, double lmbd, double eps, double* zi, void* scratch, int64_t scratch_bytes,
                    void* stream);
/* Zij (nb:200-209) and the per-edge term of avg_m_init (nb:379-392);
 * edges[2E] = G.edges (u, v) pairs, deg[n] node degrees; m_term nullable. */
int mjx_bdcm_edge_obs(const double* chi, const int32_t* edges, const int32_t* deg, int64_t E, int p, int c,
                      int attr_value, double eps, double* zij, double* m_term, void* stream);
/* The two endpoint terms of that per-edge term apart, for edge e = (u, v) with
 * its messages at rows e and e + E: m_uv[2e] = <s_u(0)>_e and m_uv[2e+1] =
 * <s_v(0)>_e, the initial spins averaged under chi^uv chi^vu / max(Zij, eps).
 * m_term[e] of mjx_bdcm_edge_obs is m_uv[2e] / deg[u] + m_uv[2e+1] / deg[v]; a
 * node's magnetisation <s_i(0)> is the mean of its terms over its edges.
 * m_uv: device [2E].  MJX_EINVAL as for mjx_bdcm_edge_obs. */
int mjx_bdcm_edge_m(const double* chi, int64_t E, int p, int c, int attr_value, double eps, double* m_uv,
                    void* stream);
/* out[0] = sum_i x[i] (take_log: sum_i log x[i]), deterministic order;
 * work: 256 doubles of device scratch. */
int mjx_sum_f64(const double* x, int64_t n, int take_log, double* work, double* out, void* stream);

/* ---- BDCM on a batch of G graphs as one disjoint union ---- */
/*
 * Instance g owns the contiguous rows [row_off[g], row_off[g] + 2 E_g) of one
 * chi[sum 2 E_g][4^T] and keeps the notebook's layout inside its block (local
 * row r < E_g is u -> v, r + E_g is v -> u), so the reverse of a union row is
 * not "row + E_total": the edge observables take both rows explicitly.  Class D
 * of the union is the union of the instances' classes D, rows / inc hold union
 * rows and inst[m] the instance of every item.  All instances share p, c,
 * attr_value, damp, eps and lambda.  Per-instance control is ctl[G][4] int64,
 * the block of mjx_bdcm_iter_* once per instance: [0] delta bits of the
 * running sweep, [1] stop flag, [2] sweeps done, [3] delta bits of the last
 * completed sweep.
 */
#define MJX_BDCM_GATE 1  /* items of an instance with ctl[g][1] != 0 are left untouched */
#define MJX_BDCM_DELTA 2 /* max |new - old| of an item's row -> atomic max into ctl[g][0] */
/* mjx_bdcm_update_class for a union class; item e belongs to instance inst[e].
 * flags: MJX_BDCM_GATE -- neither the compute nor the commit launch touches a
 * row of a stopped instance (bit for bit); MJX_BDCM_DELTA -- the maximum of
 * |new - old| over an item's row goes into its own instance's ctl[g][0] only
 * (a NaN wins).  inst and ctl are required with either flag (MJX_EINVAL) and
 * unused without.  w_dev, scratch, scratch_bytes and the chunked launches of a
 * class beyond the LDS budget as in mjx_bdcm_update_class. */
int mjx_bdcm_update_class_batch(double* chi, const int32_t* rows, const int32_t* inc, const int32_t* inst, int64_t m,
                                int D, int p, int c, int attr_value, double lmbd, double damp, double eps, double* upd,
                                long long* ctl, int flags, const double* w_dev, void* scratch, int64_t scratch_bytes,
                                void* stream);
/* mjx_bdcm_iter_begin / _end applied to each of the G control blocks
 * independently (one thread per instance). */
int mjx_bdcm_iter_begin_batch(long long* ctl, int64_t G, void* stream);
int mjx_bdcm_iter_end_batch(long long* ctl, int64_t G, double eps, int64_t t_max, void* stream);
/* mjx_bdcm_edge_obs with the two rows of union edge e given as fwd_row[e]
 * (u -> v) and rev_row[e] (v -> u); edges[2 E_total] and deg[] hold union node
 * ids.  The same summation order per edge. */
int mjx_bdcm_edge_obs_batch(const double* chi, const int32_t* fwd_row, const int32_t* rev_row, const int32_t* edges,
                            const int32_t* deg, int64_t E_total, int p, int c, int attr_value, double eps, double* zij,
                            double* m_term, void* stream);
/* out[g] = sum (take_log: sum of logs) of x[seg_ptr[g] : seg_ptr[g+1]], g < G,
 * with the bits mjx_sum_f64 gives on that segment alone; an empty segment
 * gives 0.  seg_ptr[G+1] int64 on the device; work: G*256 doubles. */
int mjx_segsum_f64(const double* x, const int64_t* seg_ptr, int64_t G, int take_log, double* work, double* out,
                   void* stream);

/* ---- flip gains and the greedy quench (no reference counterpart) --------- */
/*
 * G is an ELL or CSR graph with SYMMETRIC adjacency (as a multiset of directed
 * entries, the precondition of the light-cone calls above); row entries count
 * with multiplicity, a degree-0 node keeps its spin, the rule is sign(2S+s).
 * With T = p + c - 1, s_end = onestep^T(s), F(s) = sum s_end and s^i = s with
 * spin i flipped, for every replica r and node i:
 *   gain[r, i]   = F(s^i) - F(s): int32, even, |gain| <= 2n;
 *   consensus[r] = (F(s) = n);
 *   removable bit (i, r) = 1 iff s_i = +1, consensus[r] and F(s^i) = n; packed
 *     like the state (n * W words, W = ceil(R/64)); padding replicas stay 0;
 *   quench(s, order): every replica with consensus[r] visits i = order[0], ...,
 *     order[n-1] and, if s_i = +1 and onestep^T(s^i) is all +1, sets s <- s^i;
 *     a replica without consensus is returned unchanged; flipped[r] counts the
 *     spins turned.
 * Monotonicity: the rule is non-decreasing in every input, so s' <= s implies
 * onestep^T(s') <= onestep^T(s).  Hence (1) a node not removable in s is not
 * removable in any s' <= s; (2) one quench pass ends in a state whose
 * removable mask is empty, and a second pass flips nothing; (3) only nodes of
 * the initial removable mask can ever be flipped, so the pass visits only
 * those, in `order` order.
 *
 * levels: HOST array of T+1 device pointers, levels[t] = onestep^t(s) as
 * replica-packed words (n * W each; levels[0] = s); padding replicas 0 in all
 * of them.  caps: HOST int64 [T+1], the ball bound of the graph
 * (mjx_sa_csr_ball_bound, or mjx_ell_ball_bound = min(n, sum_{k<=t} d^k) for an
 * (n, d) neighbour array): the lists of level t never outgrow caps[t].  A wave
 * evaluates one (node, word column) pair; the first lds_entries entries of each
 * of its T+2 lists live in LDS (0 = the library's choice, 64), the rest in its
 * part of `scratch`.  mjx_quench_lds: LDS bytes of a workgroup (-1: T or
 * lds_entries out of range, more than 64 KiB).  _scratch_bytes: bytes of
 * `scratch` (always > 0: it starts with a header of 1 + 65 W words; -1 on bad
 * arguments).  After the call word 0 of `scratch` is nonzero iff a list outgrew
 * wrong caps (nothing is written out of bounds, the results are then void).
 *
 * mjx_flip_gain_*: all pairs in parallel, the levels are only read.  Writes
 * removable[n * W], consensus[R] (bytes 0 / 1) and, when `gain` is not NULL,
 * gain as int32 [n][64 W] NODE-major: gain[i * 64 W + r] (r >= R: 0).
 * mjx_quench_*: one workgroup per word column walks cand[cand_ptr[w] ..
 * cand_ptr[w+1]) (device arrays: the nodes with a removable bit in column w, in
 * `order` order) and commits every accepted flip into all T+1 levels IN PLACE
 * (the caller passes copies); writes consensus[R] (of the state as passed) and
 * flipped[64 W].
 * MJX_EINVAL: T outside 0..6, n < 1 or n >= 2^31, R < 1, a NULL required
 * pointer, scratch_bytes below _scratch_bytes.  No allocation, no host
 * synchronisation.
 */
int mjx_ell_ball_bound(int64_t n, int d, int T, int64_t* bound_out);
int64_t mjx_quench_lds(int T, int lds_entries);
int64_t mjx_flip_gain_scratch_bytes(int64_t n, int64_t R, int T, const int64_t* caps, int lds_entries);
int64_t mjx_quench_scratch_bytes(int64_t R, int T, const int64_t* caps, int lds_entries);
int mjx_flip_gain_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c,
                         const uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                         int64_t scratch_bytes, uint64_t* removable, uint8_t* consensus, int32_t* gain, void* stream);
int mjx_flip_gain_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                         const uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                         int64_t scratch_bytes, uint64_t* removable, uint8_t* consensus, int32_t* gain, void* stream);
int mjx_quench_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c, uint64_t* const* levels,
                      const int64_t* caps, int lds_entries, void* scratch, int64_t scratch_bytes,
                      const int32_t* cand, const int64_t* cand_ptr, uint8_t* consensus, int64_t* flipped,
                      void* stream);
int mjx_quench_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                      uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                      int64_t scratch_bytes, const int32_t* cand, const int64_t* cand_ptr, uint8_t* consensus,
                      int64_t* flipped, void* stream);

/* ---- the quench in rounds: region-parallel commits ------------------------ */
/*
 * The pass of mjx_quench_*_rp (definitions, levels, caps, lds_entries and the
 * overflow word of `scratch` as above) with the same result, bit for bit, by
 * the distance-2T rule.  Trying candidate i (the light cone of its flip)
 *   writes level l only within distance l of i, and only l <= T-1: an
 *     accepted replica has no level-T difference;
 *   reads level l only within distance l+2 of i (the changed nodes of level
 *     l, their rows, and the rows of those).
 * The adjacency is symmetric, so two candidates at graph distance > 2T have
 * disjoint read and write sets at every level: they commute, and either may
 * run first or both at once.  dist(i, j) <= 2T exactly when the radius-T balls
 * of i and j meet.
 *
 * cand[ncand]: device int32, the nodes with a removable bit in ANY word column
 * in `order` order (candidate k has rank k); removable: the initial mask of
 * mjx_flip_gain_* (n * W words) -- a (candidate, column) pair whose word of it
 * is 0 is not tried, as the sequential pass does not visit it.  A window of
 * `window` slots holds the pending candidates of lowest rank; everything of
 * lower rank is committed.  A round is three launches: every slot writes
 * (round, rank) with an atomic max into a per-node claim array over its
 * radius-T ball (de-duplicated, at most caps[T] nodes, walked once per
 * candidate; a later round's key beats every earlier one, nothing is reset);
 * a slot that reads its own key back on the whole ball holds the lowest rank
 * there, is ready, and hands its slot to the next candidate; a wave per (ready
 * candidate, word column) commits as mjx_quench_* does and adds to flipped
 * with integer atomics.  The pending candidate of lowest rank is always ready,
 * so ncand rounds always suffice and window = 1 is the sequential order.
 * Stream order between launches is the only synchronisation.
 *
 * One call with round0 = 0 initialises (consensus[R], flipped[64 W] zeroed,
 * the state in `scratch`, stats) and enqueues `rounds` rounds; later calls
 * with round0 = the rounds enqueued so far and the SAME other arguments
 * enqueue more.  Rounds enqueued after the end find nothing pending.  stats:
 * device int64 [4], read by the caller between calls: [0] candidates left,
 * [1] rounds that committed something, [2] the most candidates committed in
 * one round, [3] internal.  _scratch_bytes: -1 on bad arguments; it grows with
 * the window (the grid of the commit kernel is min(window * W, 8192)
 * workgroups, each with its lists, plus window * (3 + caps[T]) * 4 bytes of
 * slots and 8 n bytes of claims).
 * MJX_EINVAL: T outside 0..6, n < 1 or n >= 2^31, R < 1, window < 1, ncand
 * outside 0..n, round0 < 0, rounds < 0, a NULL required pointer (cand may be
 * NULL when ncand = 0), scratch_bytes below _scratch_bytes.  No allocation, no
 * host synchronisation.
 */
int64_t mjx_quench_regions_scratch_bytes(int64_t n, int64_t R, int T, const int64_t* caps, int lds_entries,
                                         int64_t window);
int mjx_quench_regions_ell_rp(const int32_t* adj, int64_t n, int d, int64_t R, int p, int c, uint64_t* const* levels,
                              const int64_t* caps, int lds_entries, void* scratch, int64_t scratch_bytes,
                              int64_t window, const uint64_t* removable, const int32_t* cand, int64_t ncand,
                              uint8_t* consensus, int64_t* flipped, int64_t* stats, int64_t round0, int64_t rounds,
                              void* stream);
int mjx_quench_regions_csr_rp(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int p, int c,
                              uint64_t* const* levels, const int64_t* caps, int lds_entries, void* scratch,
                              int64_t scratch_bytes, int64_t window, const uint64_t* removable, const int32_t* cand,
                              int64_t ncand, uint8_t* consensus, int64_t* flipped, int64_t* stats, int64_t round0,
                              int64_t rounds, void* stream);

/* ---- the quench as independent jobs, state in LDS ------------------------- */
/*
 * The same pass (definitions above) for R starts x K restarts: job r*K + k
 * quenches start r in its own visiting order and, for an ELL stack, on its own
 * graph.  One workgroup of one wave runs a job with the job's single replica
 * NODE-packed in LDS (bit v of a bitmap = spin of node v, as mjx_pack_np): the
 * T+1 levels, a bitmap of marks and the T+2 node lists of the light cone.  The
 * adjacency is read from global memory.  The pass walks the whole order and
 * tries every node whose spin is +1; by (3) above the result is the one of the
 * pass over the initial removable mask.
 *
 * LDS of a job: mjx_quench_jobs_lds(n, T, caps) =
 *   4 * ((T + 2) * 2 * ceil(n/64) + 1 + sum_{t=1..T} min(n, caps[t]) + min(n, caps[T]))
 * bytes rounded up to 16; -1 when T is outside 0..6, n < 1, a cap < 1, or the
 * job does not fit 64 KiB (no dynamic-LDS opt-in; n of order 1e5 at T = 3,
 * d = 4).  DECISION: a shape that does not fit is REFUSED, nothing spills to
 * caller scratch -- the bitmaps are 9/10 of the budget at the sizes that matter
 * and cannot spill, and mjx_quench_*_rp remains the path for such a shape.
 *
 * s_np: [R][ceil(n/64)] node-packed starts (padding bits ignored).  order:
 * int32 device array [R or 1][K][n], every row a permutation of 0..n-1;
 * order_stride_r = K*n, or 0 when the starts share the K orders.  ELL:
 * graph_stride = n*d for a stack adj[R][n][d] (start r on graph r), 0 for one
 * shared graph.  CSR: shared graph only.  caps as above; with a stack, of every
 * graph of it (mjx_ell_ball_bound depends on n and d alone).
 * Outputs, all on the device: out_np[R*K][ceil(n/64)] with padding bits 0,
 * flipped[R*K], plus[R*K] (+1 spins of the result), consensus[R] (bytes 0 / 1,
 * of the start), flag[R*K]: 0, or bit 0 = a list outgrew wrong caps, bit 1 = an
 * order or adjacency entry outside 0..n-1; such a job stops, writes nothing out
 * of bounds, and its results are void.  A start without consensus comes back
 * unchanged with flipped = 0 in each of its K jobs.
 * MJX_EINVAL: T outside 0..6, n < 1 or n >= 2^31, R < 1, K < 1, R*K >= 2^31, a
 * NULL pointer, strides other than the above, a shape that does not fit.  No
 * allocation, no host synchronisation.
 */
int64_t mjx_quench_jobs_lds(int64_t n, int T, const int64_t* caps);
int mjx_quench_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R, int64_t K, int p, int c,
                        const int64_t* caps, const uint64_t* s_np, const int32_t* order, int64_t order_stride_r,
                        uint64_t* out_np, int64_t* flipped, int64_t* plus, uint8_t* consensus, int32_t* flag,
                        void* stream);
int mjx_quench_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K, int p, int c,
                        const int64_t* caps, const uint64_t* s_np, const int32_t* order, int64_t order_stride_r,
                        uint64_t* out_np, int64_t* flipped, int64_t* plus, uint8_t* consensus, int32_t* flag,
                        void* stream);

/* ---- the (1, 2) exchange descent behind the quench jobs -------------------- */
/*
 * A quench ends in a single-flip local minimum.  The smallest move that leaves
 * one downwards is a (1, 2) exchange: turn one -1 spin to +1 (consensus is
 * kept, the rule is monotone), then drop two +1 spins.  Per job (start r, order
 * k; jobs, orders, graphs, s_np, caps and the first outputs as mjx_quench_jobs_*),
 * with consensus(z) = "onestep^T(z) is all +1":
 *
 *   x = start
 *   if not consensus(x): result = start, flipped = exchanges = passes = 0,
 *                        converged = 1
 *   x = the quench pass over ord (flipped = its count); plus_quench = +1 spins of x
 *   for pass = 1 .. max_passes:
 *       moved = false
 *       for j in ord, with x[j] = -1 at its turn:
 *           y = x with y[j] = +1; dropped = 0
 *           for a in ord, a != j, y[a] = +1 at its turn:
 *               if consensus(y with y[a] = -1): y[a] = -1, dropped += 1
 *           if dropped >= 2: x = y, exchanges += 1, moved = true
 *           (dropped = 1, a swap of equal weight, and dropped = 0 leave x as it was)
 *       passes = pass
 *       if not moved: converged = 1, stop
 *
 * converged = the last pass committed nothing (the greedy inner walk can take a
 * single drop that blocks a pair, so it does not say that no pair exists).  x
 * stays a single-flip local minimum; every exchange lowers the weight by at
 * least 1.  T = 0 returns the start (passes = 1 with consensus).
 *
 * The kernel tries fewer nodes with the same result (DESIGN.md has the proof):
 * with D_t the nodes whose level-t value the add of j changed (t < T; D_0 =
 * {j}), only a +1 node within t + 2 hops of some D_t can be dropped after the
 * add that could not be dropped before.  These candidates lie in the ball of
 * radius 2T around j; cap2T bounds that ball (mjx_ell_ball_bound(n, d, 2T)[2T]
 * or mjx_sa_csr_ball_bound(.., 2T)[2T]; both serve radius <= 6, so T <= 3) and
 * the list of min(n, cap2T) entries joins the job's LDS:
 *   mjx_quench_exchange_jobs_lds(n, T, caps, cap2T) =
 *     mjx_quench_jobs_lds(n, T, caps) + 4 * min(n, cap2T), rounded up to 16;
 *   -1 as mjx_quench_jobs_lds, for T > 3, cap2T < 1, or past the same 64 KiB.
 * rank_work: device int32 [R*K*n], workspace (a job's inverse order; need not
 * be initialised).  max_passes >= 1.  Further outputs, device arrays [R*K]:
 * plus_quench (+1 spins after the quench pass), exchanges, passes (int64),
 * converged (bytes 0 / 1).  flag: bits 0 and 1 as above (a candidate list past
 * cap2T counts as bit 0), bit 2 = a flip that restores the state after an add
 * without two drops did not commit (a bug, never an input error).  stats: NULL,
 * or device int64 [R*K][4] = adds tried, candidate drops tried, and the device's
 * constant-rate clock ticks of the quench phase and of the passes.
 * MJX_EINVAL: as mjx_quench_jobs_*, T > 3, max_passes < 1, cap2T < 1, a NULL
 * pointer other than stats.  No allocation, no host synchronisation.
 */
int64_t mjx_quench_exchange_jobs_lds(int64_t n, int T, const int64_t* caps, int64_t cap2T);
int mjx_quench_exchange_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R, int64_t K,
                                 int p, int c, const int64_t* caps, int64_t cap2T, int max_passes,
                                 const uint64_t* s_np, const int32_t* order, int64_t order_stride_r,
                                 int32_t* rank_work, uint64_t* out_np, int64_t* flipped, int64_t* plus,
                                 int64_t* plus_quench, int64_t* exchanges, int64_t* passes, uint8_t* converged,
                                 uint8_t* consensus, int32_t* flag, int64_t* stats, void* stream);
int mjx_quench_exchange_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K, int p,
                                 int c, const int64_t* caps, int64_t cap2T, int max_passes, const uint64_t* s_np,
                                 const int32_t* order, int64_t order_stride_r, int32_t* rank_work, uint64_t* out_np,
                                 int64_t* flipped, int64_t* plus, int64_t* plus_quench, int64_t* exchanges,
                                 int64_t* passes, uint8_t* converged, uint8_t* consensus, int32_t* flag,
                                 int64_t* stats, void* stream);

/* ---- Metropolis add / drop inside the consensus set ------------------------ */
/*
 * Every pass above is a descent and stops at the first state its move set
 * cannot leave.  This one walks INSIDE the consensus set at a finite
 * temperature: Metropolis on the up-set {z : consensus(z)}, consensus(z) =
 * "onestep^T(z) is all +1", T = p + c - 1, with energy = the weight (number of
 * +1 spins) and inverse temperature beta_u in sweep u.  A drop that keeps
 * consensus lowers the energy and is always taken, a drop that leaves the set
 * is refused, an add (never leaves the set: the rule is monotone) is taken with
 * probability e^{-beta_u}.  It is the chain of code/SA_RRG.py in the limit
 * b -> infinity, started inside the set instead of stopping at its border.
 *
 * Per job (start r, restart k; jobs, orders, graphs, s_np, caps and the first
 * outputs as mjx_quench_jobs_*), with a 64-bit seed, sweeps = U >= 0 and a
 * device array thr of U uint32:
 *
 *   x = start
 *   if not consensus(x): result = start; flipped = 0;
 *                        plus_quench = plus_best = plus(start); best_sweep = 0;
 *                        adds = drops = refused = 0; trace[u] = plus(start)
 *   x = the quench pass over ord (flipped = its count); plus_quench = plus(x)
 *   best = x; plus_best = plus_quench; best_sweep = 0
 *   for u = 0 .. U-1:
 *       for q = 0 .. n-1:
 *           (w0, w1, _, _) = philox4x32_10(counter = (q, u, r, k),
 *                                          key = (seed & 0xffffffff, seed >> 32))
 *           i = (w0 * n) >> 32                        (64-bit product)
 *           if x[i] = +1: if consensus(x - i): x = x - i, drops += 1
 *                         else refused += 1
 *           else:         if w1 < thr[u]:     x = x + i, adds += 1
 *       trace[u] = plus(x)
 *       if plus(x) < plus_best: best = x; plus_best = plus(x); best_sweep = u + 1
 *   result = the quench pass over ord from best; plus = plus(result)
 *
 * thr[u] = min(floor(e^{-beta_u} * 2^32), 2^32 - 1), computed by the caller in
 * float64: the device evaluates no exponential and the results are bit-exact.
 * The counter holds (r, k), not the job index, so a job keeps its stream
 * whatever R and K are.  The result is a consensus single-flip local minimum;
 * plus <= plus_best <= plus_quench, so a job is never worse than the same job
 * of mjx_quench_jobs_*; U = 0 gives exactly that call's output.  T = 0:
 * consensus is "all +1", every proposal is refused.
 *
 * One wave runs a job; its LDS is the quench job's plus one bitmap, the
 * snapshot `best`:
 *   mjx_quench_anneal_jobs_lds(n, T, caps) =
 *     mjx_quench_jobs_lds(n, T, caps) + 4 * 2 * ceil(n/64), rounded up to 16;
 *   -1 as mjx_quench_jobs_lds, or past the same 64 KiB.
 * T = 0..6 as mjx_quench_jobs_* (no ball of radius 2T is needed).
 * Further outputs, device arrays: plus_quench, plus_best, best_sweep int64
 * [R*K]; moves int64 [R*K][3] = adds, drops, refused; trace NULL or int32
 * [R*K][U].  flag: bits 0 and 1 as mjx_quench_jobs_*, bit 2 = an accepted add
 * did not commit (a bug, never an input error).  The results of a flagged job
 * are void; its trace is written only up to the sweep before the one it
 * stopped in, the rest is left as the caller passed it.
 * MJX_EINVAL: as mjx_quench_jobs_*, sweeps < 0 or >= 2^31, thr NULL with
 * sweeps > 0, a NULL output other than trace, a shape that does not fit.  No
 * allocation, no host synchronisation.
 */
int64_t mjx_quench_anneal_jobs_lds(int64_t n, int T, const int64_t* caps);
int mjx_quench_anneal_jobs_ell(const int32_t* adj, int64_t n, int d, int64_t graph_stride, int64_t R, int64_t K, int p,
                               int c, const int64_t* caps, int64_t sweeps, const uint32_t* thr, uint64_t seed,
                               const uint64_t* s_np, const int32_t* order, int64_t order_stride_r, uint64_t* out_np,
                               int64_t* flipped, int64_t* plus, int64_t* plus_quench, int64_t* plus_best,
                               int64_t* best_sweep, int64_t* moves, int32_t* trace, uint8_t* consensus, int32_t* flag,
                               void* stream);
int mjx_quench_anneal_jobs_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t R, int64_t K, int p,
                               int c, const int64_t* caps, int64_t sweeps, const uint32_t* thr, uint64_t seed,
                               const uint64_t* s_np, const int32_t* order, int64_t order_stride_r, uint64_t* out_np,
                               int64_t* flipped, int64_t* plus, int64_t* plus_quench, int64_t* plus_best,
                               int64_t* best_sweep, int64_t* moves, int32_t* trace, uint8_t* consensus, int32_t* flag,
                               void* stream);

/* ---- exact consensus census of a small graph ------------------------------- */
/*
 * Ground truth by exhaustive enumeration: every start configuration of a graph
 * of n <= 48 nodes is run T = p + c - 1 steps (0 <= T <= 6, the rule of the
 * quench calls) and counted when it has reached all +1.  G is an ELL (n, d) or
 * CSR graph with symmetric adjacency, the always-stay majority rule of the
 * sweeps (sign(2S+s), row entries count with multiplicity), a node of degree 0
 * keeps its spin; a row holds at most 47 entries.
 *   Configuration index: x in [0, 2^n); node v is +1 iff bit v of x is set; the
 *     weight is k(x) = popcount(x).
 *   64-config block: block b holds x = 64 b .. 64 b + 63; there are
 *     B = 2^max(n-6, 0) blocks.  For n < 6 only the first 2^n bit positions of
 *     block 0 are configurations; the rest is masked out.
 *   Counts: for t = 0..T, counts[t][k] = #{x : k(x) = k and onestep^t(x) is all
 *     +1}.  All +1 is a fixed point of the rule, so counts[t] <= counts[t+1]
 *     elementwise; counts[0] is 1 at k = n and 0 elsewhere.  One enumeration
 *     gives the whole dependence on p.
 *   Witness: for each t the configuration with the smallest (k(x), x) in
 *     lexicographic order among those counted in counts[t], as the key
 *     k(x) << 48 | x.  It does not depend on the launch geometry or on how the
 *     range of blocks is split.
 *
 * A lane owns one block at a time and walks a grid-stride loop over
 * [block_lo, block_hi); the configurations are generated in place (node v < 6
 * is a constant bit pattern, node v >= 6 is all ones iff bit v-6 of b is set),
 * so nothing is read from memory but the adjacency.  The workgroup is one wave;
 * its LDS holds two levels as [node][lane] words, its counts and keys, the
 * level-0 patterns and the adjacency: mjx_census_lds(n) =
 *   1024 n + 56 (n + 2) + 8 n + 8 ceil((n + 1) / 4) + 8 ceil(47 n / 8)
 * bytes (-1 for n outside 1..48; 54,696 at n = 48, no dynamic-LDS opt-in).
 *
 * counts: device [T+1][n+1], ADDED to (64-bit atomics); witness_key: device
 * [T+1], atomic-min'ed into (the caller starts it at all ones; a level nobody
 * reaches keeps that value); so a caller may split [0, B) over several launches
 * into the same buffers.  flag: one device int32 the caller zeroes, OR'ed into:
 * bit 1 = an adjacency entry outside 0..n-1, bit 2 = a CSR row longer than 47
 * entries or a row_ptr that does not start at 0 or decreases; the kernel then
 * stops in bounds and the results are void.  grid: 0 = the library's choice,
 * > 0 forces the number of workgroups.  block_lo = block_hi does nothing.
 * MJX_ERANGE: n > 48, T > 6, d > 47.  MJX_EINVAL: n < 1, p or c < 0, T < 0, a
 * block range outside 0 <= block_lo <= block_hi <= B, grid < 0, a NULL pointer.
 * No allocation, no host synchronisation.
 */
int64_t mjx_census_lds(int64_t n);
int mjx_census_ell(const int32_t* adj, int64_t n, int d, int p, int c, int64_t block_lo, int64_t block_hi, int grid,
                   unsigned long long* counts, unsigned long long* witness_key, int32_t* flag, void* stream);
int mjx_census_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t block_lo,
                   int64_t block_hi, int grid, unsigned long long* counts, unsigned long long* witness_key,
                   int32_t* flag, void* stream);

/* ---- census marginals: the counts of one level per node -------------------- */
/*
 * mjx_census_nodes_ell / _csr: mjx_census_ell / _csr (same enumeration, counts,
 * witness keys, flag and status codes) that also counts the configurations of
 * ONE level t_node, 0 <= t_node <= T, per +1 node:
 *   Node counts: node_counts[k][v] = #{x : k(x) = k, bit v of x set and
 *     onestep^t_node(x) is all +1}, (n+1, n).  So sum_v node_counts[k][v] =
 *     k counts[t_node][k], node_counts <= counts[t_node], and at t_node = 0 the
 *     row k = n is all ones and the rest 0.
 *   Backbone: with k* = min_plus[t_node], node v is +1 in every optimal
 *     configuration iff node_counts[k*][v] = counts[t_node][k*] and -1 in every
 *     one iff node_counts[k*][v] = 0.
 * The workgroup keeps node[n+1][n] as 32-bit LDS cells behind its counts and
 * keys and flushes them with 64-bit global atomics at the end; a launch covers
 * at most 2^25 blocks (2^31 configurations), so no cell can wrap.  The word of
 * a lane's block is binned by weight as for the counts; node v < 6 takes the
 * positions of its level-0 pattern, node v >= 6 the whole word where bit v-6 of
 * b is set.  In a row of 64 blocks that starts at a multiple of 64 the bits
 * v >= 12 are the same in every lane: the wave's words are summed by weight
 * once and lane l adds the sums for node 12 + l.  mjx_census_nodes_lds(n) =
 *   mjx_census_lds(n) + 4 (n + 1) n
 * bytes (-1 for n outside 1..48; 64,104 at n = 48, no dynamic-LDS opt-in).
 *
 * node_counts: device [n+1][n], ADDED to (64-bit atomics), like counts: [0, B)
 * may be split over launches into the same buffers.  When the flag comes back
 * set, nothing has been counted.  MJX_ERANGE: as for mjx_census_*, and
 * block_hi - block_lo > 2^25.  MJX_EINVAL: as for mjx_census_*, and t_node
 * outside 0..T.  No allocation, no host synchronisation.
 */
int64_t mjx_census_nodes_lds(int64_t n);
int mjx_census_nodes_ell(const int32_t* adj, int64_t n, int d, int p, int c, int t_node, int64_t block_lo,
                         int64_t block_hi, int grid, unsigned long long* counts, unsigned long long* witness_key,
                         unsigned long long* node_counts, int32_t* flag, void* stream);
int mjx_census_nodes_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int t_node,
                         int64_t block_lo, int64_t block_hi, int grid, unsigned long long* counts,
                         unsigned long long* witness_key, unsigned long long* node_counts, int32_t* flag,
                         void* stream);

/* ---- census of the minimal consensus sets -------------------------------- */
/*
 * The rule is monotone, so U_t = {x : onestep^t(x) is all +1}, the set that
 * counts[t] counts, is an up-set: raising a spin keeps x in it.  Its minimal
 * elements are the local minima of a greedy quench at T = t: consensus
 * configurations from which no single +1 node can be dropped.  With
 * T = p + c - 1 and t = 0..T:
 *   Mask: mask[t][b] is a 64-bit word; bit j is set iff configuration
 *     x = 64 b + j is in U_t.  For n < 6 only the first 2^n bits of block 0 can
 *     be set.  Layout (T+1, B) words, B = 2^max(n-6, 0): (T+1) 2^n / 8 bytes,
 *     2 GiB at n = 32, T = 3.
 *   Minimal set: M_t = {x in U_t : x without i is not in U_t for every +1 node
 *     i of x}; minima[t][k] = #{x in M_t : popcount(x) = k}.
 *   Heaviest minimum: for each t the x in M_t with the largest (popcount(x), x),
 *     as the key k << 48 | x under an atomic max.  The key starts at 0, which
 *     no minimum has: all -1 is a fixed point and never reaches all +1.
 *   Lightest minimum: the witness of the census.
 * So minima[t][min_plus[t]] = counts[t][min_plus[t]], minima[t] <= counts[t]
 * elementwise, and minima[0] is 1 at k = n and 0 elsewhere.
 *
 * Pass 1, mjx_census_mask_ell / _csr: mjx_census_ell / _csr (same enumeration,
 * counts, witness keys, flag and status codes) that also stores the word of
 * every block b of [block_lo, block_hi) at mask[t B + b] for every t = 0..T,
 * one plain vector store per lane and level -- the zero words and the full
 * blocks the enumeration does not sweep included, so the caller does not
 * zero the buffer.  mask: device [(T+1) B] words, NULL is MJX_EINVAL.  When
 * the flag comes back set the mask is void like the counts.
 *
 * Pass 2, mjx_census_minima, needs no graph: it counts the minimal elements of
 * the levels of any such bitmap whose levels are up-sets.  A wave owns 64
 * consecutive blocks (lane = the low six bits of b) and looks x without node v
 * up inside its own word (v < 6), in the word of lane ^ 2^(v-6) (v < 12) and in
 * the 64 consecutive words at (b & ~63) ^ 2^(v-6) (v >= 12, one coalesced
 * 512-byte row, read only where that bit of b is set); a wave whose 64 words
 * are all zero at a level reads nothing more.  A block reads only blocks of
 * lower index, at most 2^(n-3) (1 + (n-12)/2) bytes per level; they must
 * have been written, whatever range this call covers.
 * minima: device [T+1][n+1], ADDED to (64-bit atomics); heaviest_key: device
 * [T+1], atomic-max'ed into (the caller starts it at 0); so [0, B) may be
 * split over launches into the same buffers.  A wave's 64 blocks go together:
 * block_lo must be a multiple of 64 and block_hi a multiple of 64 or B.
 * grid: 0 = the library's choice (a resident grid-stride loop), > 0 forces the
 * number of one-wave workgroups.  MJX_ERANGE: n > 48, T > 6.  MJX_EINVAL: n < 1,
 * T < 0, a block range outside 0 <= block_lo <= block_hi <= B or not aligned
 * as above, grid < 0, a NULL pointer.  No allocation, no host synchronisation.
 */
int mjx_census_mask_ell(const int32_t* adj, int64_t n, int d, int p, int c, int64_t block_lo, int64_t block_hi,
                        int grid, unsigned long long* counts, unsigned long long* witness_key, int32_t* flag,
                        uint64_t* mask, void* stream);
int mjx_census_mask_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int p, int c, int64_t block_lo,
                        int64_t block_hi, int grid, unsigned long long* counts, unsigned long long* witness_key,
                        int32_t* flag, uint64_t* mask, void* stream);
int mjx_census_minima(const uint64_t* mask, int64_t n, int T, int64_t block_lo, int64_t block_hi, int grid,
                      unsigned long long* minima, unsigned long long* heaviest_key, void* stream);

/* ---- attractor census: where all 2^n starts of a small graph end up -------- */
/*
 * The census above looks at a fixed horizon and at one outcome; this one runs
 * every start configuration to its attractor.  Graph, rule, configuration
 * index x, weight k = popcount(x) and 64-config blocks as for mjx_census_*.
 *   Trajectory: s(0) = x, s(t+1) = onestep(s(t)).
 *   p = min{t >= 0 : s(t+2) = s(t)}, c = 1 if s(p+1) = s(p), else 2 -- the
 *     definitions of mjx_attractor_record, exactly.
 *   Class of x:  0 plus   c = 1 and s(p) is all +1
 *                1 minus  c = 1 and s(p) is all -1
 *                2 fixed  c = 1, neither of the above
 *                3 cycle  c = 2
 *     A configuration with p > t_max is unsettled and belongs to no class.
 *   hist[class][p][k], (4, t_max+1, n+1): the number of x of weight k in that
 *     class with transient exactly p.  unsettled[k], (n+1).  Per weight they
 *     add up to C(n, k).  The cumulative sum of hist[0] over p <= t is
 *     counts[t] of the census, for every horizon t <= t_max.
 *   keys[0], lightest_plus: the smallest (k, x) over class plus, any p, as
 *     k << 48 | x under an atomic min (the caller starts it at all ones; all +1
 *     is in the class, so a full enumeration always finds one).
 *   keys[1], longest: the largest (p, x) over the settled configurations, as
 *     p << 48 | x under an atomic max (the caller starts it at 0, which is the
 *     key of all -1: a fixed point, p = 0, x = 0; a range without a settled
 *     configuration leaves the word alone).
 *   Neither key depends on the launch geometry or the split of the range.
 *
 * The frame of the census kernel: a lane owns one block at a time, level 0 is
 * generated, the adjacency sits in LDS as bytes, the workgroup is one wave.
 * Two LDS level buffers: sweep t reads s(t-1) from one and writes s(t) over
 * s(t-2) in the other, comparing with both before the store.  A wave sweeps
 * until each of its 64 x 64 configurations has settled, at most t_max + 2
 * times.  The workgroup's counts are 32-bit LDS cells flushed with 64-bit
 * global atomics at the end; a launch covers at most 2^25 blocks (2^31
 * configurations), so no cell can wrap.  mjx_attractor_census_lds(n, t_max) =
 *   1024 n + 16 (t_max + 1)(n + 1) + 8 ceil((n + 1) / 2) + 16 + 8 n
 *   + 8 ceil((n + 1) / 4) + 8 ceil(47 n / 8)
 * bytes: 52,176 at n = 32, t_max = 32; -1 for n outside 1..48, t_max outside
 * 0..1024, or more than 65,536 bytes (no dynamic-LDS opt-in).
 *
 * hist, unsettled: device, ADDED to (64-bit atomics); keys: device [2] as
 * above; so [0, B) may be split over launches into the same buffers.  flag: as
 * for mjx_census_* (bit 1 = an adjacency entry outside 0..n-1, bit 2 = a bad
 * CSR row); the kernel then stops in bounds and writes nothing else.  stats:
 * NULL, or device [2] ADDED to: the 64-block rows the waves ran and the sweeps
 * they made (sweeps / rows = the mean number of sweeps of a wave).  grid: 0 =
 * the library's choice, > 0 forces the number of workgroups.
 * MJX_ERANGE: n > 48, t_max > 1024, d > 47, block_hi - block_lo > 2^25.
 * MJX_EINVAL: n < 1, t_max < 0, an LDS demand past 65,536 bytes, a block range
 * outside 0 <= block_lo <= block_hi <= B, grid < 0, a NULL pointer (stats
 * excepted).  No allocation, no host synchronisation.
 */
int64_t mjx_attractor_census_lds(int64_t n, int t_max);
int mjx_attractor_census_ell(const int32_t* adj, int64_t n, int d, int t_max, int64_t block_lo, int64_t block_hi,
                             int grid, unsigned long long* hist, unsigned long long* unsettled,
                             unsigned long long* keys, int32_t* flag, unsigned long long* stats, void* stream);
int mjx_attractor_census_csr(const int64_t* row_ptr, const int32_t* col, int64_t n, int t_max, int64_t block_lo,
                             int64_t block_hi, int grid, unsigned long long* hist, unsigned long long* unsettled,
                             unsigned long long* keys, int32_t* flag, unsigned long long* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MJX_H */

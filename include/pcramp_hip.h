/*
 * pcramp_hip.h -- C-ABI of the MI355X-native primer-pair x target evaluation path.
 *
 * The reference (LANL-Bioinformatics/PCRamp v0.3) has no plugin/FFI layer: its boundary for
 * this path is a set of C++ member functions called from main.cpp / optimize.cpp.  Each entry
 * point below replaces the reference call sites it cites (file:line under the reference tree)
 * and is what a `pcramp` host driver binds instead of them.
 *
 * Conventions: C linkage, opaque handle, plain pointers + sizes, caller-owned buffers, `int`
 * status (0 = ok, <0 = error; text via pcr_last_error(), thread-local).  No exceptions cross
 * the ABI.  A handle owns one GPU and one HIP stream and is not thread-safe (the reference's
 * equivalent rule: one NucCruc / SeqOverlap per OpenMP thread, main.cpp:533,702): it is used from
 * one thread at a time.  The library runs one helper thread of its own per (device, stream) on which
 * pcr_screen_device is used -- it stages and launches the passes the caller's thread has planned --
 * shared by the handles created on that stream, started by their first such pass and joined when
 * the last of them is destroyed.  It never calls back into the caller's code, and every entry point
 * first waits for it to have launched the handle's queued passes (see pcr_screen_device;
 * PCRAMP_LAUNCH_THREAD=0 at pcr_create: no helper thread, the caller's thread launches).
 * There is NO CPU fallback: every compute entry point fails if no gfx950 device is usable.
 */
#ifndef PCRAMP_HIP_H
#define PCRAMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_OK               0
#define PCR_ERR_ARG         -1
#define PCR_ERR_DEVICE      -2   /* no usable GPU / HIP failure */
#define PCR_ERR_STATE       -3   /* call order (e.g. amplify before select) */
#define PCR_ERR_CAPACITY    -4   /* a fixed device buffer would overflow even after growth */
#define PCR_ERR_RANGE       -5   /* reference `throw` conditions (e.g. Sequence::has_split out of bounds) */

typedef struct pcr_ctx pcr_ctx;

/* Reference `Word` (= __word<unsigned long,2>, word.h:690): 32 slots of 4-bit IUPAC codes,
 * slot k (0 = 5' end) at bits (15 - k%16)*4 of w[k/16]; A=1 C=2 G=4 T=8, EOS=0 (base_table.h:11-28). */
typedef struct { uint64_t w[2]; } pcr_word128;

/* One trial assay: PCR::f / PCR::r (assay.h:117-118). */
typedef struct { pcr_word128 f, r; } pcr_pair;

/* The sequence sets of a context: target_seq, background_seq (main.cpp:257-344) and multiplex_background_seq, the amplicons of
 * the assays accepted so far as sequences (main.cpp:989-1001; templates of find_multiplex_background_match). */
typedef enum { PCR_SET_TARGET = 0, PCR_SET_BACKGROUND = 1, PCR_SET_MULTIPLEX = 2 } pcr_set;
#define PCR_N_SETS 4   /* + one internal scratch set */

/* The `Options` fields (pcramp.h:83-128) that Sequence::pack reads (sequence.cpp:92-96). */
typedef struct {
	uint32_t pack_max_degen;  /* opt.pack_max_degen, default 256 (pcramp.h:43) */
	float pack_min_gc;        /* opt.pack_min_gc, default 0 = off (pcramp.h:45) */
	float pack_max_gc;        /* opt.pack_max_gc, default 1 = off (pcramp.h:44) */
} pcr_params;

/* One entry of the per-iteration word DB (`MULTIMAP<Word, WordMatch>`, sequence.h:34-76). */
typedef struct {
	pcr_word128 word;
	int32_t loc;       /* WordMatch::loc */
	uint32_t index;    /* WordMatch::index (sequence index inside its set) */
	uint32_t strand;   /* 1 = Seq_strand_plus, 2 = Seq_strand_minus (sequence.h:27-32) */
	uint32_t pad;
} pcr_entry;

/* Arguments of the amplicon screen; mirrors what PCR::collect_candidates (pcr_assay.cpp:12-18)
 * and PCR::find_target_match / compute_coverage (pcr_assay.cpp:544,271) take from `Options`. */
typedef struct {
	float collect_threshold;  /* m_threshold of collect_candidates: target_threshold (find_target_match,
	                             pcr_assay.cpp:556) or target_threshold*search_multiplier (assay.h:407);
	                             squared inside, as pcr_assay.cpp:31-32 */
	float ident_threshold;    /* the sqrtf(f*r) >= threshold test (pcr_assay.cpp:574, :294) */
	int32_t amp_min, amp_max; /* m_amplicon_range (pcramp.h:14-18) */
	int32_t use_taq_mama;     /* opt.use_taq_mama (optimize.cpp:209) */
} pcr_amplify_args;

const char *pcr_last_error(void);

/* Device index + an optional caller HIP stream (hipStream_t as void*, NULL = create one).
 * Fails (returns NULL) when no gfx950 device is available. */
pcr_ctx *pcr_create(int device, void *hip_stream, const pcr_params *params);
void pcr_destroy(pcr_ctx *ctx);

/* Replaces the host-resident `deque<Sequence>` (main.cpp:257-344 after parse_fasta):
 * `packed4` holds the sequences' 4-bit codes, high nibble first (sequence.h:223-228);
 * sequence i starts at byte byte_offsets[i] and has lengths[i] bases; weights[i] = Sequence::weight().
 * Builds the HBM-resident bit-plane store, the window-validity mask (the degeneracy / GC /
 * EOS filters of Sequence::pack, sequence.cpp:127-153) and the irregular word list (centred
 * partial words at sequence ends and around EOS, sequence.cpp:155-179,198-263). */
int pcr_load_sequences(pcr_ctx *ctx, pcr_set which, const uint8_t *packed4,
	const uint64_t *byte_offsets, const uint64_t *lengths, const float *weights, uint32_t n);

/* Sequence::active(bool) for every sequence of the set (main.cpp:1105-1120); active[i] != 0 = active. */
int pcr_set_active(pcr_ctx *ctx, pcr_set which, const uint8_t *active);

/* Sequence::split_sequence (sequence.h:228-241; main.cpp:1008-1017): write EOS at `pos`. */
int pcr_split(pcr_ctx *ctx, pcr_set which, uint32_t seq, uint64_t pos);
/* n splits at once (the three per amplicon of an accepted assay, main.cpp:1008-1017: a few hundred per design iteration): the
 * derived device state -- window validity around each split, the set's irregular word list -- is refreshed once. */
int pcr_split_many(pcr_ctx *ctx, pcr_set which, const uint32_t *seq, const uint64_t *pos, uint32_t n);

/* The per-iteration index build, main.cpp:579-615 / 644-691: for every ACTIVE sequence
 * Sequence::pack (sequence.cpp:92) + select_words (select_words.cpp:8) with the trial assays
 * `pairs`; the result (the set's word DB) stays on the device.  `threshold` is the
 * select_words m_threshold (target_threshold*target_search_multiplier, main.cpp:669; not squared);
 * `min_oligo_length` is the pack argument (opt.min_oligo_length(), x0.9 for backgrounds, main.cpp:595).
 * n_entries_out (optional) receives the DB size. */
int pcr_select_words(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	int optimize_5, int optimize_3, float threshold, uint32_t min_oligo_length,
	uint64_t *n_entries_out);

/* The all-sites fill of a set's word DB: EVERY binding site of each oligo, not the best per sequence.
 * pcr_select_words keeps, per (oligo, sequence), only the words that attain the maximum match count (the threshold is a
 * floor, select_words.cpp:100-117); a weaker site on a sequence that also holds a better site of the same oligo does not
 * exist for the consumers of that DB.  This call fills the DB the way the reference fills its multiplex DB (pack, then
 * match_words, main.cpp:989-1001): for every ACTIVE sequence of `which`, every entry Sequence::pack(min_oligo_length) emits
 * -- regular windows on both strands, the centred partial words at the sequence ends and around EOS, under the handle's
 * degeneracy / GC filters -- is kept when at least one oligo c of the batch (F and R of every pair; no 5'/3' shift
 * candidates) has (c & word) >= unsigned(c.size()*threshold), the float product and truncation of select_words.cpp:83.
 * The result REPLACES the set's word DB in the layout pcr_select_words leaves (entries unique, per sequence ordered by
 * (loc, strand, kind, ord)), so pcr_get_entries, pcr_amplify, pcr_collect_amplicons, pcr_pool_products,
 * pcr_background_match, pcr_move_coverage, ... read it as they read a selected DB.  n_entries_out as pcr_select_words.
 *   - Synchronous; pending pcr_screen_device passes are drained first (their buffers are final when this call returns).
 *   - Errors as pcr_select_words (PCR_ERR_ARG: unknown set, min_oligo_length outside [1,32] -- checked before the handle --,
 *     NULL handle, NULL pairs with n_pairs > 0); PCR_SET_MULTIPLEX is refused with PCR_ERR_ARG.
 *   - n_pairs == 0 or an empty set: an empty DB, PCR_OK.
 *   - The per-sequence buckets grow and shrink on the ladder of pcr_select_words (64 ... 65 536 slots; a window that
 *     several oligos match counts once per strand and launch group of 128 pairs).  More sites than that in one sequence,
 *     or buckets that would not fit the device: PCR_ERR_CAPACITY, the set is left without a DB and its buckets start
 *     at 64 slots again.
 *   - On a handle with a target shard attached (pcr_shard_targets) the call works on this rank's block and makes no
 *     collective, as pcr_collect_amplicons.
 *   - The consumers floor at collect_threshold SQUARED (pcr_assay.cpp:31-32).  To give a consumer that will be called
 *     with threshold t every site it could use, pass (float)t*(float)t here. */
int pcr_select_sites(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	float threshold, uint32_t min_oligo_length, uint64_t *n_entries_out);

/* Copy the current word DB to the host (parity tests; the reference's target_db). Returns the
 * number of entries (may exceed cap; only cap are written) or <0. */
int64_t pcr_get_entries(pcr_ctx *ctx, pcr_set which, pcr_entry *out, uint64_t cap);

/* The amplicon screen for a batch of pairs against every sequence of the set:
 * PCR::collect_candidates + update_identity + the sqrtf(f*r) test, i.e. PCR::find_target_match
 * (pcr_assay.cpp:544-578) and PCR::compute_coverage (pcr_assay.cpp:271-302) in one pass.
 *   bits      : n_pairs x pcr_bitset_words(ctx,which) u64 words, bit (i%64) of word i/64 = sequence i
 *               amplified by the pair (BitSet, bitset.h:7).  May be NULL.
 *   bits_fr   : same shape, amplified through {F(+),R(-)} (pcr_assay.cpp:39-45).  May be NULL.
 *   bits_rf   : same shape, amplified through {R(+),F(-)} (pcr_assay.cpp:52-58).  May be NULL.
 *   coverage  : n_pairs floats = compute_coverage's return value (double sum in the reference's
 *               amplicon order, then rounded to float).  May be NULL. */
int pcr_amplify(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	const pcr_amplify_args *args, uint64_t *bits, uint64_t *bits_fr, uint64_t *bits_rf,
	float *coverage);

/* Same screen, asynchronous on the handle's stream, results left in DEVICE memory
 * (d_bits_fr / d_bits_rf: n_pairs x words each, caller-allocated, e.g. a torch tensor that is
 * then all-gathered over RCCL).  No host synchronisation. */
int pcr_amplify_device(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	const pcr_amplify_args *args, uint64_t *d_bits_fr, uint64_t *d_bits_rf);

/* pcr_select_words followed by pcr_amplify_device for the same batch -- one optimiser iteration's
 * DB build + find_target_match (main.cpp:644-691 then pcr_assay.cpp:544-578) -- ENQUEUED on the
 * handle's stream without any host wait, so the host plans pass i+1 while pass i runs.
 * The per-sequence bucket overflow that pcr_select_words handles by retrying cannot be seen
 * before the pass has run: the device buffers are final only after pcr_synchronize() (or any other
 * entry point of the same handle) has returned PCR_OK -- that call inspects the counters of every
 * enqueued pass and, if a pass overflowed, replays it and the later ones with larger buckets into
 * the same buffers.  At most 6 passes are kept in flight.
 * Threading: the call returns once the pass is QUEUED -- planned on the calling thread and handed to the
 * stream's launcher thread, which writes its tables to the device and launches its kernels, in call order
 * across all handles of the stream.  `pairs` and `args` are copied before the call returns; the two device
 * buffers must stay valid until pcr_synchronize.  Stream order holds against later calls of this library
 * only: synchronize (or call any other entry point of the handle) before enqueuing work of your own on
 * the stream that reads the buffers.  An error met while launching (HIP, capacity) is returned by the
 * NEXT call on the handle, with its text in that thread's pcr_last_error(); the handle's passes queued
 * behind the failed one are dropped, not launched.  Passes that cannot be planned without device work (the
 * first over a set, 5'/3' shift candidates, first-form tables, a tail that is not fused) run inline.
 * Pairs: a queued pass may wait on the launcher thread for the next pass of ANOTHER handle of the stream and
 * share its two launches with it (PCRAMP_PAIR=0: never); it waits only while the GPU still has two passes
 * to start, and any call that has to wait for the handle's queued passes releases it.  So the bits of a
 * pass are there to be read only after pcr_synchronize (or any other entry point) of its handle has
 * returned: a stream or device synchronisation alone does not launch a pass that is still queued. */
int pcr_screen_device(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	int optimize_5, int optimize_3, float select_threshold, uint32_t min_oligo_length,
	const pcr_amplify_args *args, uint64_t *d_bits_fr, uint64_t *d_bits_rf);

/* One local-search move, evaluated as optimize_pcr.cpp does for each of its six moves (e.g.
 * increase_degeneracy :57-100; the loop of optimize(), optimize.cpp:120-140, calls them per oligo):
 * the candidate amplicons are those of the BASE pair -- collected at args->collect_threshold
 * (= target_threshold*search_multiplier, optimize.cpp:61-63, assay.h:405-408) against the word DB of
 * the last pcr_select_words -- and for every variant of the edited oligo (side 0 = F, 1 = R) only that
 * oligo's identity table is recomputed (update_identity, optimize.cpp:209-261: the variant's own
 * length and 3' bases) before compute_coverage at args->ident_threshold (pcr_assay.cpp:271-302).
 *   variants  : n_variants trial words (as the move leaves them, not re-centred)
 *   bits_fr / bits_rf : n_variants x pcr_bitset_words u64, per orientation as pcr_amplify.  May be NULL.
 *   coverage  : n_variants floats = compute_target_coverage of each trial.  May be NULL. */
int pcr_move_coverage(pcr_ctx *ctx, pcr_set which, const pcr_pair *base, int side,
	const pcr_word128 *variants, uint32_t n_variants, const pcr_amplify_args *args,
	uint64_t *bits_fr, uint64_t *bits_rf, float *coverage);

/* compute_coverage's weight sum (pcr_assay.cpp:280-301) from gathered orientation bitsets:
 * ascending index over bits_fr, then ascending index over bits_rf & ~bits_fr, accumulated in
 * double; n = number of sequences, weights[n].  Pure host arithmetic (no device needed). */
float pcr_coverage_from_bits(const uint64_t *bits_fr, const uint64_t *bits_rf,
	const float *weights, uint64_t n);

/* weighted_coverage (main.cpp:1402-1418): ascending-index double sum of weights over set bits. */
float pcr_weighted_coverage(const uint64_t *bits, const float *weights, uint64_t n);

uint32_t pcr_num_sequences(pcr_ctx *ctx, pcr_set which);
uint64_t pcr_bitset_words(pcr_ctx *ctx, pcr_set which);   /* ceil(n/64) */

/* Measurement hooks (bench.py): when enabled, the dominant kernel of pcr_select_words (the
 * oligo x window match scan) is bracketed by HIP events on the handle's stream.  on = 1: every pass;
 * on = n > 1: every n-th pass (an event packet between two kernels costs a ~6 us queue bubble).
 * pcr_profile_read: total milliseconds and number of bracketed launches since the last reset. */
int pcr_profile_enable(pcr_ctx *ctx, int on);
int pcr_profile_read(pcr_ctx *ctx, double *scan_ms, uint64_t *scan_launches, int reset);
/* The same for the other kernels bench.py prices: while profiling is on, EVERY launch of the Smith-Waterman kernel
 * (k_sw) and of the thermodynamics kernels is bracketed by HIP events on the handle's stream. */
#define PCR_PROF_SCAN    0   /* = pcr_profile_read */
#define PCR_PROF_SW      1
#define PCR_PROF_THERMO  2
#define PCR_PROF_KERNELS 3
int pcr_profile_read_kernel(pcr_ctx *ctx, int kernel, double *ms, uint64_t *launches, int reset);

/* Blocks until the handle's stream is idle. */
int pcr_synchronize(pcr_ctx *ctx);

/* How the small per-pass tables of pcr_screen_device reach the device (reported by bench.py): 1 = "lean" -- the CPU
 * stores them straight into fine-grained device memory (large BAR; probed by pcr_create with a store / fence / kernel
 * read-back round trip) and the pass has no staging launch; 0 = a staging kernel (k_stage) copies them out of mapped
 * host memory (PCRAMP_STAGE=kernel, no large BAR, or a failed probe). */
int pcr_staging_mode(pcr_ctx *ctx);

/* How many pcr_screen_device passes of this handle went through its stream's launcher thread (the others ran
 * inline on the calling thread), and the largest number of them queued there at once.  Either pointer may be NULL. */
int pcr_launcher_stats(pcr_ctx *ctx, uint64_t *passes_pipelined, uint32_t *max_queue_depth);

/* What the handles of this process hold on the device right now: out[0] = bytes of device memory, out[1] = bytes of host-mapped
 * pinned memory, out[2] = HIP events, out[3] = streams the library created itself (a stream passed to pcr_create is borrowed and
 * not counted).  Process-wide and needs no handle; all four are back at their earlier values once a handle is destroyed. */
int pcr_live_resources(uint64_t out[4]);

/* ---- multi-GPU: the path's one exchange step.  Targets shard across ranks (one process per GPU,
 * contiguous blocks whose boundaries are multiples of 64 sequences, so every rank owns whole bitset words); the primer pairs are
 * replicated; after a pass every rank needs every rank's orientation bitsets.  This replaces what the reference's MPI mode does
 * with its per-rank best assay -- Send/Recv of the BitSets to rank 0 and MPI_Bcast of the winner (main.cpp:1421-1601; wire
 * format mpi_util.cpp:152-233) -- by ONE ncclAllGather over xGMI, enqueued on the handle's stream (no host hop, no torch).
 *   pcr_comm_unique_id   rank 0: 128 opaque bytes (RCCL's ncclUniqueId) to hand to every rank (the reference's MPI_Bcast, a file, ...)
 *   pcr_comm_init_rank   every rank, once: joins the communicator with this handle's device (any handle on that device may then
 *                        exchange through it); NULL + pcr_last_error() on failure
 *   pcr_exchange_bits    every rank, per pass: all-gather of words_per_rank u64 from d_local (device) into d_full (device,
 *                        world x words_per_rank, rank-major).  Waits on the host only for the counters of passes pcr_screen_device
 *                        enqueued (a bucket overflow replays a pass into the same buffers), then enqueues the collective; the
 *                        result is complete after pcr_synchronize / in stream order for later kernels on the handle's stream.
 * Coverage is then pcr_coverage_from_bits on every rank over the gathered words, in the reference's summation order.
 * RCCL is bound at run time (the copy already loaded in the process first; PCRAMP_RCCL=<path> overrides). */
#define PCR_COMM_ID_BYTES 128
typedef struct pcr_comm pcr_comm;
int pcr_comm_unique_id(uint8_t id[PCR_COMM_ID_BYTES]);
pcr_comm *pcr_comm_init_rank(pcr_ctx *ctx, const uint8_t id[PCR_COMM_ID_BYTES], int world, int rank);
int pcr_comm_world(const pcr_comm *comm);
int pcr_comm_rank(const pcr_comm *comm);
int pcr_exchange_bits(pcr_ctx *ctx, pcr_comm *comm, const uint64_t *d_local, uint64_t words_per_rank, uint64_t *d_full);
void pcr_comm_destroy(pcr_comm *comm);
const char *pcr_comm_library(void);      /* which librccl was bound ("" before the first use / when none was found) */

/* A host-collective communicator: every exchange goes through fn, an all-gather the caller provides -- `bytes` from `send` on
 * every rank into `recv`, world x bytes in rank order, host memory; 0 = ok.  It is how an MPI program binds the library
 * (MPI_Allgather), and how two ranks share one GPU (RCCL refuses that).  pcr_exchange_bits on it copies
 * device -> host, calls fn and copies host -> device; pcr_comm_world / _rank / _destroy take both kinds. */
typedef int (*pcr_host_allgather_fn)(const void *send, uint64_t bytes, void *recv, void *user);
pcr_comm *pcr_comm_init_host(pcr_ctx *ctx, int world, int rank, pcr_host_allgather_fn fn, void *user);

/* ---- the local search over targets sharded across ranks (pcr_shard.inc)
 * pcr_shard_targets: the loaded PCR_SET_TARGET holds rows [first_seq, first_seq + n) of n_total targets spread over comm, in
 * rank order (boundaries at any index).  Collective: one all-gather checks that the ranges are contiguous in rank order and
 * cover n_total (else PCR_ERR_ARG on every rank) and picks the combine.  comm = NULL detaches (not collective); reloading the
 * target set detaches too; the communicator must outlive the attachment.  With a shard attached:
 *   pcr_optimize_batch / pcr_optimization_move  combine every trial word's target coverage over the ranks, bit-exact with the
 *       reference's compute_coverage (pcr_assay.cpp:271-302: weights summed in double, ascending global sequence index, the
 *       F(+)/R(-) bits first, then the R(+)/F(-) bits not yet counted, cast to float).  Backgrounds and the multiplex set are
 *       whole on every rank and not combined.  All ranks must call with the same batch (checked: PCR_ERR_ARG on every rank).
 *   pcr_make_degenerate  gathers every rank's candidate amplicons and merges them into the reference's order (order_amplicons:
 *       by pair, orientation, global sequence, plus site, minus site) before the unchanged walk.
 *   pcr_design  runs the design loop over the shard once the handle is design-ready (pcr_shard_sampler_targets below); before
 *       that it returns PCR_ERR_STATE at once, on each rank by itself (no collective).  Every rank must then call it with the
 *       same arguments, command line and pcr_output describing all n_total targets (checked: PCR_ERR_ARG on every rank); every
 *       rank leaves the same text and the same pool, equal to the unsharded call on the whole set.  Rank 0 samples the trials
 *       over its host copy and sends them; select / amplify run over local rows, the best assay's bits and amplicons are gathered.
 * A failure on one rank (incl. the has_split range error) is returned by every rank; no rank leaves a collective out.
 * pcr_shard_combine_mode: 0 = not sharded, 1 = exact partials (every partial sum is exactly representable in double, so one
 * all-gather of per-rank sums per iteration is exact), 2 = ordered chain (the reference's sequential sum, rank after rank, 2 x world
 * all-gathers per iteration).  PCRAMP_SHARD_COMBINE=auto|exact|chain, read at attach time: auto and exact take 1 where it is
 * provably exact, else 2. */
int pcr_shard_targets(pcr_ctx *ctx, pcr_comm *comm, uint64_t first_seq, uint64_t n_total);
int pcr_shard_combine_mode(pcr_ctx *ctx);

/* pcr_shard_gather_bits: collective over the attached shard.  d_local (device): n_vec bitsets over this rank's n rows, row i at bit
 * i%64 of word i/64, bitset v at d_local + v*local_stride_words; d_global (device, every rank): the same n_vec bitsets over all
 * n_total rows at d_global + v*global_stride_words, bits at or past n_total zero (the whole stride is written).  Boundaries may
 * lie anywhere (pcr_exchange_bits needs multiples of 64).  One agreement on n_vec, one all-gather of padded records (on the
 * handle's stream over RCCL; device -> host -> fn -> device over a host communicator), then k_shard_stitch on the stream; returns
 * after the result is complete.  A bad argument on any rank: PCR_ERR_ARG on every rank; no shard attached: PCR_ERR_STATE. */
int pcr_shard_gather_bits(pcr_ctx *ctx, const uint64_t *d_local, uint32_t n_vec, uint64_t local_stride_words,
	uint64_t *d_global, uint64_t global_stride_words);

/* pcr_shard_sampler_targets: collective; makes the handle design-ready.  Rank 0 passes the whole target set packed as for
 * pcr_load_sequences (n == n_total), every other rank n = 0 and null pointers.  The copy stays on the host (0.5 B per base) and
 * is what rank 0's sampler of pcr_design walks; one all-gather checks it against every rank's rows (lengths and a hash of the
 * bytes).  A mismatch, a wrong n or rank 0 passing nothing: PCR_ERR_ARG on every rank.  Detaching, re-attaching or reloading
 * the target set drops the copy and the design-ready flag. */
int pcr_shard_sampler_targets(pcr_ctx *ctx, const uint8_t *packed4, const uint64_t *byte_offsets, const uint64_t *lengths, uint64_t n);

/* ---- the design loop in the reference's MPI mode: trials split across ranks (pcr_trial_ranks.inc)
 * pcr_design_trial_ranks: attaches comm (RCCL, pcr_comm_init_rank, or a host all-gather, pcr_comm_init_host).  Every rank has
 * loaded the same TARGET and BACKGROUND sets.  Collective: one all-gather checks count, lengths, a hash of the packed bytes (EOS
 * splits included), weights and active flags of both sets; a mismatch gives PCR_ERR_ARG on every rank.  With a target shard
 * attached it returns PCR_ERR_STATE at once (and pcr_shard_targets returns PCR_ERR_STATE while trial ranks are attached): the two
 * modes do not combine.  comm = NULL detaches (not collective); reloading either set detaches too; the communicator must outlive
 * the attachment.  While attached, pcr_design is collective and runs as `mpirun -np W pcramp` does (main.cpp:60-113, :926-932,
 * :1420-1601):
 *   - on entry the ranks agree on the arguments, command line, pcr_output sizes and the sets' state (PCR_ERR_ARG on every rank
 *     when they differ);
 *   - args->num_trial is the trials of THIS rank (the caller divides as main.cpp:65 does: max(1, ceil(num_trial / W))); the
 *     sampler's running seed starts at args->seed + rank (unsigned wrap); the header still prints args->seed;
 *   - every rank runs the one-rank iteration over its own trials; after the walk, and before the `target coverage <= 0` stop, one
 *     all-gather of a fixed-size record per rank (status, Score, assay, background bits) reduces the ranks' best assays: rank 0's
 *     is the starting best, then in ascending rank order a record replaces it iff it scores higher, or ties with a lower
 *     total degeneracy (the reference's root takes the ranks in arrival order);
 *   - the winner's target bits and amplicons depend on the word DB only the winning rank built, so that rank computes them and a
 *     second exchange ships them (as the reference does); the rest of the iteration (record text, multiplex set, EOS splits, active
 *     flags, pool) is the one-rank code on every rank.
 * Every rank leaves the output file the reference's root writes and the same pool.  Any rank's failure (the sampler's throws
 * included) is returned as the same code by every rank; no rank leaves a collective out.  PCRAMP_TIMING=1 reports the exchanges
 * as "reduction".  Without an attachment pcr_design is unchanged.
 * pcr_design_trial_world: the attached world size, 0 when nothing is attached. */
int pcr_design_trial_ranks(pcr_ctx *ctx, pcr_comm *comm);
int pcr_design_trial_world(pcr_ctx *ctx);


/* ---- Smith-Waterman primer x template alignment (rows a7/a8 of the scope table) */

/* Outputs of one SO::SeqOverlap lane (seq_overlap.h:1266-1330). */
typedef struct {
	int16_t score;              /* SeqOverlap::score() = max_elem.M */
	int16_t q_start, q_stop;    /* alignment_range_query() */
	int16_t t_start, t_stop;    /* alignment_range_target() */
	uint8_t last1, last2;       /* target_last_two_aligned() (15,15 = N,N when undefined) */
	uint8_t valid;              /* 0: no cell reached the running maximum; the reference leaves the
	                               coordinates stale then, here they are zero and only score (0) is defined */
	uint8_t pad;
} pcr_sw_result;

/* n independent alignments, query word i against template word i, exactly as
 * SeqOverlap::pack_query_slots / pack_target_slots(Word) + align() (SmithWaterman, nucleic acid)
 * evaluate one lane (seq_overlap.h:828,1099; seq_overlap.cpp:347-609). */
int pcr_sw_align_words(pcr_ctx *ctx, const pcr_word128 *queries, const pcr_word128 *templates, uint32_t n,
	pcr_sw_result *out);

typedef struct {
	float collect_threshold;     /* background_threshold*background_search_multiplier (assay.h:418); squared inside */
	float background_threshold;  /* the final score test (background_match.cpp:116) */
	int32_t amp_min, amp_max;    /* opt.background_amplicon_range */
	int32_t use_taq_mama;
	int32_t evaluate_all_amplicons;  /* 0 (default): reference-identical -- see below; 1: every candidate amplicon counts */
} pcr_background_args;

/* PCR::find_background_match (background_match.cpp:7-166) for a batch of pairs against the set's
 * current word DB: candidate amplicons -> 4 alignments each -> normalised score product ->
 * bits[pair][seq].
 * The reference aligns its candidate amplicons two per SeqOverlap call (:66-75) and tests
 * `(i + 1) >= num_seq` (:122, the number of SEQUENCES, not of amplicons) before scoring the second one:
 * in the order collect_candidates leaves them (pcr_assay.cpp:39-58: {F(+),R(-)} first, then {R(+),F(-)},
 * each by sequence, plus site, minus site) an amplicon with an odd index >= the set's sequence count is
 * never scored.  With evaluate_all_amplicons = 0 that is reproduced bit for bit; with 1 every candidate
 * amplicon is scored.  (One case stays ours in both modes: an odd amplicon COUNT below num_seq makes the
 * reference score stale SSE lanes and index past its deque -- undefined there, no extra amplicon here.)
 * Pairs per call: the pairing kernel holds 8 bytes per pair in the LDS of a workgroup beside about 8 KB of its own,
 * so a call takes at most (LDS a workgroup of the device may declare - the kernel's own) / 8 pairs: about 19 400
 * on an MI355X (160 KiB).  More is refused before anything is launched with PCR_ERR_CAPACITY and
 * "pcr_background_match: too many pairs in one call: at most <N> pairs ..."; bits is untouched and the handle
 * stays usable.  Split a larger batch.
 * With PCRAMP_DEBUG set, every attempt of a call writes one "[pcramp] background_match:" line to stderr (form of the
 * pairing kernel, bucket slots, pairs, list and sub-list capacity, records emitted and kept, overflow, how it ended). */
int pcr_background_match(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	const pcr_background_args *args, uint64_t *bits);

/* PCR::find_multiplex_background_match (background_match.cpp:168-295): F, (F), R, (R) of every
 * pair aligned against every whole sequence of the set (amplicon sequences, up to 32766 bases: the
 * reference's own limit -- SeqOverlap counts columns in a 16-bit integer up to and including the
 * template length and never returns at 32767); bit set when any single normalised score reaches the
 * threshold.  bits receives n_pairs x ceil(n / 64) words, bits at or past n zero; nothing is written
 * for an empty set or zero pairs.  A set holding a longer template is refused with PCR_ERR_CAPACITY:
 * bits is then all zero, and the handle stays usable. */
int pcr_multiplex_match(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs,
	float background_threshold, int use_taq_mama, uint64_t *bits);

/* ---- Nearest-neighbour thermodynamics (rows a9/a10 of the scope table) */

/* The `Options` fields the thermodynamic filters read (pcramp.h:21-30). */
typedef struct {
	float salt;            /* opt.salt -> NucCruc::salt() (main.cpp:535) */
	float primer_strand;   /* opt.primer_strand */
	float tm_min, tm_max;  /* opt.primer_tm_range */
	float max_hairpin;     /* opt.max_hairpin */
	float max_dimer;       /* opt.max_dimer */
} pcr_thermo_args;

typedef struct {
	uint32_t valid;        /* PCR::is_valid(): every IUPAC expansion passes all enabled tests */
	uint32_t n_expansions; /* Word::degeneracy() as an integer */
	float tm, dH, dS;      /* NucCruc::tm_pm_duplex / delta_H / delta_S of the FIRST expansion (Word::begin()); kcal/mol, kcal/(mol K) */
	float hairpin_tm;      /* approximate_tm_hairpin of the first expansion */
	float homodimer_tm;    /* approximate_tm_homodimer of the first expansion (0 unless check_homo_dimer) */
	float dG;              /* NucCruc::delta_G() = dH - 310.15 K * dS of the perfect-match duplex (nuc_cruc.h:1375-1378), first expansion */
} pcr_thermo_result;

/* PCR::is_valid (valid_pcr.cpp:5-45) for n oligos: perfect-match duplex Tm in [tm_min, tm_max],
 * hairpin Tm <= max_hairpin and, if check_homo_dimer, homodimer Tm <= max_dimer, for every
 * non-degenerate expansion, at strand concentration primer_strand/degeneracy (valid_pcr.cpp:13). */
int pcr_thermo(pcr_ctx *ctx, const pcr_word128 *oligos, uint32_t n, int check_homo_dimer,
	const pcr_thermo_args *args, pcr_thermo_result *out);

/* PCR::is_valid without the dimer test (valid_pcr.cpp:5-31) for n words: valid_out[i] = 1 iff every expansion of
 * words[i] has its perfect-match duplex Tm in [tm_min, tm_max] and its hairpin Tm <= max_hairpin, at strand
 * concentration primer_strand/degeneracy.  The same verdicts as pcr_thermo with check_homo_dimer = 0, by the path the
 * local search takes for its trial words: one record per word, the expansions spelt and the verdict reduced on the
 * device.  Errors as pcr_thermo: PCR_ERR_ARG for an empty word, a hole between the oligo's ends or a length over 32,
 * PCR_ERR_CAPACITY for more than 65536 expansions. */
int pcr_valid_words(pcr_ctx *ctx, const pcr_word128 *words, uint32_t n, const pcr_thermo_args *args,
	uint8_t *valid_out);

/* PCR::max_dimer_tm (pcr_assay.cpp:232-269): max heterodimer Tm of F x R over all expansions,
 * strand(primer_strand/D(F), primer_strand/D(R)) (nuc_cruc.h:818-838). */
int pcr_dimer(pcr_ctx *ctx, const pcr_pair *pairs, uint32_t n, const pcr_thermo_args *args, float *max_tm);

/* PCR::multiplex_compatible (pcr_assay.cpp:815-852): ok[i] = 1 iff no oligo expansion of assay
 * a[i] forms a heterodimer with any oligo expansion of assay b[i] at Tm >= max_dimer
 * (strand = primer_strand, no degeneracy correction). */
int pcr_multiplex_compatible(pcr_ctx *ctx, const pcr_pair *a, const pcr_pair *b, uint32_t n,
	const pcr_thermo_args *args, uint8_t *ok);

/* ---- Multiplex background (the third coverage term of the multiplex local search) */

/* The multiplex background DB and its keys (main.cpp:989-1001): every word Sequence::pack emits for the
 * amplicon sequences of the assays accepted so far (pack_max_degen of pcr_create, no G+C filter,
 * min_oligo_length = opt.min_oligo_length()), made unique.  The call REPLACES the key table: pass all amplicons
 * collected so far.  Sequence format as pcr_load_sequences.  n_keys_out (optional) = keys(db).size(). */
int pcr_multiplex_load(pcr_ctx *ctx, const uint8_t *packed4, const uint64_t *byte_offsets, const uint64_t *lengths,
	uint32_t n, uint32_t min_oligo_length, uint64_t *n_keys_out);

/* collect_multiplex_background_candidates (pcr_assay.cpp:71-102) for `base`, then, for every trial word of the
 * oligo on `side` (0 = F, 1 = R), update_identity of that oligo's map (optimize.cpp:209-261) and
 * compute_multiplex_background_coverage (pcr_assay.cpp:304-336): coverage[v] = number of distinct candidate
 * keys whose identity with the forward or with the reverse oligo is >= background_threshold.  The unedited
 * assay is the variant `base->f` (side 0). */
int pcr_multiplex_coverage(pcr_ctx *ctx, const pcr_pair *base, int side, const pcr_word128 *variants, uint32_t n_variants,
	float background_threshold, int use_taq_mama, float *coverage);

/* One amplicon an assay produces on a sequence of the set (AmpliconBounds, assay.h:64-89, plus the stretch
 * extract_amplicon_seq spells for the multiplex background, pcr_assay.cpp:489-497). */
typedef struct {
	uint32_t sequence;               /* AmpliconBounds::index */
	int32_t  begin, end;             /* first / last base of the amplicon INCLUDING both primers */
	int32_t  inner_start;            /* first base of the stretch that becomes a multiplex background sequence ... */
	int32_t  inner_length;           /* ... and its length (non-primer part + MULTIPLEX_AMPLICON_PADDING) */
	uint32_t orientation;            /* 0: F on the plus strand, 1: R on the plus strand */
} pcr_amplicon;

/* PCR::collect_unique_amplicons (pcr_assay.cpp:756-813; main.cpp:787,920) for one assay over the word DB of the
 * last pcr_select_words on `which`: every (plus site, minus site) pair of an active sequence whose oligos match
 * at threshold^2, do not overlap, span amp_min..amp_max bases and enclose no EOS.  Records sorted by
 * (orientation, sequence, begin, end).  Returns the number found (may exceed cap; only cap are written) or a
 * negative error.  The caller cuts the strings from its Sequences, makes them unique (sort + unique, :805-806),
 * passes them to pcr_multiplex_load and splits the targets at begin, (begin+end)/2 and end (main.cpp:1008-1017). */
int64_t pcr_collect_amplicons(pcr_ctx *ctx, pcr_set which, const pcr_pair *pair, float threshold, int32_t amp_min, int32_t amp_max,
	pcr_amplicon *out, uint64_t cap);

/* ---- Cross-assay products of a primer pool */

/* One product two oligos of a pool form on a sequence of the set (32 bytes). */
typedef struct {
	uint32_t plus_oligo, minus_oligo;   /* distinct-oligo ids (see oligo_id) in the plus- and the minus-strand role */
	uint32_t sequence;
	int32_t  begin, end;                /* as pcr_amplicon */
	int32_t  inner_start, inner_length; /* as pcr_amplicon */
	uint32_t intended;                  /* 1: some pool pair i has {id(F_i), id(R_i)} = {plus_oligo, minus_oligo} */
} pcr_product;

#define PCR_POOL_MAX_PAIRS 1024     /* 2 048 distinct oligos */

/* Every amplicon any two oligos of a pool form over the word DB of the last pcr_select_words on `which`.
 * The pool's 2*n_pool oligo words (F of pair i is slot 2i, R is slot 2i+1) get distinct ids in order of first
 * appearance; oligo_id[2*n_pool] receives them.  For every ordered pair of distinct oligos (x, y), x = y included, the
 * products are the amplicons PCR::collect_unique_amplicons / extract_amplicon_seq (pcr_assay.cpp:443-542,756-813) admit
 * with x in the plus-strand role and y in the minus-strand role: both sites match at threshold^2, the plus site's sequence
 * is active, the sites do not overlap, amp_min <= end - begin + 1 <= amp_max, and the inner stretch lies inside the
 * sequence and holds no EOS -- what pcr_collect_amplicons reports for the pair (x, y) in orientation 0.  So for oligos a
 * and b, pcr_collect_amplicons((a, b)) gives the products (a, b) as orientation 0 and (b, a) as orientation 1; for a = b
 * it gives each product twice, this call once.  Records are unique by (plus_oligo, minus_oligo, sequence, begin, end) and
 * sorted by that key.  Returns the number of products or a negative error; if it exceeds cap, the contents of out are
 * unspecified (cap = 0: count only).  n_pool = 0 returns 0.  PCR_ERR_STATE without a word DB; PCR_ERR_ARG for
 * PCR_SET_MULTIPLEX, null pointers or n_pool > PCR_POOL_MAX_PAIRS.  Changes nothing other calls read.  On a handle with
 * a target shard attached, sequence indices are local to the rank's block and no collective is made (as
 * pcr_collect_amplicons). */
int64_t pcr_pool_products(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, uint32_t *oligo_id, pcr_product *out, uint64_t cap);

/* ---- Per-site duplex Tm: every binding site of a panel's oligos in the word DB, melted */

/* One binding site of one oligo (48 bytes). */
typedef struct {
	uint32_t oligo;                     /* distinct-oligo id (see oligo_id) */
	uint32_t sequence;
	int32_t  loc5, loc3;                /* WordMatch::template_loc5 / template_loc3 (sequence.h:57-75) with the oligo's start() / stop() */
	uint32_t strand;                    /* 1: the oligo in the plus-strand role (a product's begin side), 2: minus */
	uint32_t matches;                   /* slots of the oligo the site's word matches: Word & Word of the entry the target is read from */
	uint32_t n_expansions;              /* non-degenerate expansions of the oligo (Word::degeneracy()) */
	uint32_t flags;                     /* PCR_SITE_* */
	float    tm_max, tm_min;            /* highest / lowest heterodimer Tm over the expansions, degrees C */
	float    dH, dS;                    /* NucCruc::delta_H / delta_S of the expansion that attains tm_max (the lowest-numbered one on a tie) */
} pcr_site;

#define PCR_SITE_NO_TM 1u               /* the site's template bases cannot be spelled in A, C, G, T: every float is 0 */
#define PCR_SITE_MAX_EXPANSIONS 256     /* an oligo with more expansions is refused */

/* Every binding site of every distinct oligo of a panel over the word DB of the last pcr_select_words or pcr_select_sites
 * on `which`, with the duplex Tm of the oligo against the template strand it anneals to there.
 *   Sites.  The panel's 2*n_pairs oligo words get distinct ids in order of first appearance, as in pcr_pool_products;
 * oligo_id[2*n_pairs] receives them.  A site of oligo c is a (sequence, loc, strand) of the DB, strand 1 or 2, sequence
 * active, at which some entry e has (e.w & c) >= unsigned(c.size() * threshold * threshold) -- the sites pcr_pool_products
 * forms its products from.  loc5 / loc3 are template_loc5 / template_loc3 of that entry with c.start() / c.stop(): a
 * product's begin is its plus site's loc5 and its end is its minus site's loc3, exactly (the entries' own loc is used as it
 * is, including the + 1 that Sequence::pack gives the partial words at a sequence's tail).
 *   Template bases.  They are read from the entry's word, not from the sequence.  T = slots c.start() - 1 .. c.stop() + 1
 * clipped to 0 .. 31: the oligo's slots and one flanking slot on either side where the word has one (NucCruc turns a
 * flanking base into a dangling end).  Where several entries share the site and match c, the one with the most occupied
 * slots in T is read (on a tie the one whose slot masks (A, C, G, T) compare lowest); `matches` is that entry's count.
 * Empty slots are dropped from both ends of T.  If a slot left is empty or holds more than one base, flags =
 * PCR_SITE_NO_TM and tm_max = tm_min = dH = dS = 0.  Otherwise the target is the complement of those bases read from the
 * highest slot to the lowest: the 5'->3' spelling of the strand the oligo anneals to.
 *   What a caller must know about EOS splits.  No word of the DB has an empty slot inside: Word::push_back writes the next
 * base over an EOS (word.cpp:32-41), so a word over a pcr_split joins the bases on either side of it.  The empty-slot half
 * of the rule above is therefore never met on a DB this library builds, and PCR_SITE_NO_TM in practice means an ambiguity
 * code.  A site straddling a split is reported as the weaker site its joined word is, with the Tm of a target that does
 * not exist in the template as one molecule, and WITHOUT a flag: a caller that splits sequences and cares must compare
 * loc5 .. loc3 with its own split positions.
 *   Thermodynamics.  For each non-degenerate expansion q of c in the order of Word::begin() / next():
 * NucCruc::approximate_tm_heterodimer with query q, that target, salt = args->salt and
 * strand(args->primer_strand / c.degeneracy(), template_strand) by the two-concentration rule (nuc_cruc.h:818-838);
 * template_strand = 0 is legal.  Only salt and primer_strand of args are read.
 *   Records are unique and sorted by (oligo, sequence, loc5, strand).  Returns their number or a negative error; if it
 * exceeds cap the contents of out are unspecified (cap = 0: count only, no thermodynamics is run).  n_pairs = 0 returns 0.
 * PCR_ERR_ARG (checked before the handle): unknown set or PCR_SET_MULTIPLEX, null pointers, n_pairs > PCR_POOL_MAX_PAIRS,
 * a negative concentration or a zero strand concentration of a duplex (primer_strand and template_strand both 0), salt
 * outside [1e-6, 1], an oligo that is empty, has a hole between its ends or more than
 * PCR_SITE_MAX_EXPANSIONS expansions; then a null handle.  PCR_ERR_STATE without a word DB; PCR_ERR_CAPACITY for 2^31 or
 * more sites or (site, expansion) jobs.  Changes nothing other calls read.  On a handle with a target shard attached,
 * sequence indices are local to the rank's block and no collective is made (as pcr_pool_products). */
int64_t pcr_site_tm(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	const pcr_thermo_args *args, float template_strand, uint32_t *oligo_id, pcr_site *out, uint64_t cap);

/* ---- A panel's binding sites grouped by what the template spells there */

/* One distinct spelling of the template under (and beside) one oligo (80 bytes). */
typedef struct {
	pcr_word128 word;                   /* planes of the entry pcr_site_tm reads for the site, restricted to T (the oligo's slots and one
	                                       flanking slot on either side, clipped to 0..31), as a Word: oligo-oriented on both strands */
	uint32_t oligo;                     /* distinct-oligo id, pcr_pool_products' numbering */
	uint32_t sites;                     /* sites (pcr_site_tm records) of this oligo that spell it */
	uint32_t sequences;                 /* distinct `sequence` values among them */
	uint32_t matches;                   /* as pcr_site.matches (the same for every member) */
	uint32_t mismatch_mask;             /* bit i: the oligo's slot start+i (i = 0: its 5' base) matches no base of the word there */
	uint32_t clamp3, clamp5;            /* consecutive matching slots counted from slot stop downwards / from slot start upwards */
	uint32_t n_expansions;
	uint32_t flags;                     /* PCR_SITE_NO_TM, pcr_site_tm's rule */
	uint32_t first_sequence; int32_t first_loc5; uint32_t first_strand;   /* the member lowest in (sequence, loc5, strand) */
	float    tm_max, tm_min, dH, dS;    /* pcr_site_tm's, bit for bit, for every member; all 0 with args == NULL or NO_TM */
} pcr_site_variant;

/* A census of a panel's binding sites by what the template spells at them: how many sites and sequences carry each spelling,
 * where it mismatches the oligo, and -- melted once per spelling, not once per site -- its Tm.
 *   Sites.  Exactly the records pcr_site_tm returns for the same handle state, `which`, panel and threshold, with the same
 * entry read where several share a site; oligo_id[2*n_pairs] receives the same ids.
 *   Variants.  The key of a site is (oligo, the read entry's planes & T), T as at pcr_site_tm.  DB words are oligo-oriented
 * on both strands, so strand is no part of the key: a strand-1 and a strand-2 site with the same word are one variant.
 * Two oligos never share a variant; an oligo that occurs several times in the panel is one oligo.  The grouping compares
 * whole keys (radix sorts, no hash): it is exact.  pcr_site_tm spells both strands of a site's duplex from the oligo and
 * from those planes alone, so tm_max, tm_min, dH, dS, matches and flags of a variant are, bit for bit, those of every
 * pcr_site_tm record among its members.  clamp3 / clamp5 equal the oligo's length where nothing mismatches; a slot of the
 * oligo over an empty slot of the word (a site hanging over a sequence end) counts as a mismatch.
 *   Thermodynamics.  args != NULL: one duplex per (variant, expansion) by pcr_site_tm's rules (salt, primer_strand /
 * degeneracy, template_strand, highest Tm with the lowest expansion on a tie).  args == NULL: none is run, the four floats
 * are 0, template_strand is ignored and the salt and concentration checks are skipped; flags is still computed.
 *   Records are sorted by oligo ascending, then sequences, sites and matches descending, then the word's slot masks
 * (A, C, G, T) ascending: a total order.  Returns their number or a negative error; if it exceeds cap the contents of out
 * are unspecified (cap = 0: count only, no thermodynamics is run).  n_pairs = 0 returns 0.
 *   site_variant (may be NULL): entry r receives the index in out of the variant of the r-th record of pcr_site_tm's
 * order (oligo, sequence, loc5, strand); written iff the variants fit cap and the sites fit site_cap.  counts (may be
 * NULL): counts[0] = the number of sites, written by every successful call; counts[1] = the number of (variant,
 * expansion) duplexes melted, the sum of n_expansions over the variants, or 0 where no thermodynamics ran.  counts[1] is
 * at most the sum of n_expansions over pcr_site_tm's records, and equal to it iff no two sites share a variant.
 *   PCR_ERR_ARG (checked before the handle): pcr_site_tm's refusals in its order, args == NULL being legal; then site_cap > 0
 * with site_variant == NULL; then a null handle.  PCR_ERR_STATE without a word DB; PCR_ERR_CAPACITY for 2^31 or more sites
 * or (variant, expansion) duplexes; PCR_ERR_RANGE for an internal trace-back failure.  Changes nothing other calls read.  On
 * a handle with a target shard attached, sequence indices are local to the rank's block and no collective is made. */
int64_t pcr_site_variants(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	const pcr_thermo_args *args, float template_strand, uint32_t *oligo_id,
	pcr_site_variant *out, uint64_t cap,
	uint32_t *site_variant, uint64_t site_cap, uint64_t counts[2]);

/* ---- Degenerate bases that win back a panel's eroded binding sites */

#define PCR_REPAIR_MAX_STEPS      12     /* a plain oligo gains at most 12 (slot, base) bits within 256 expansions: 4*4*4*4 */
#define PCR_REPAIR_MAX_CANDIDATES 4096
#define PCR_REPAIR_COMPLETE   1u         /* every sequence with a site of the oligo is held */
#define PCR_REPAIR_NO_GAIN    2u         /* the best candidate wins no sequence, or nothing can be unioned for another reason */
#define PCR_REPAIR_DEGENERACY 4u         /* unheld single-base variants exist, but every union exceeds max_degeneracy */
#define PCR_REPAIR_STEPS      8u         /* max_steps steps were taken */
#define PCR_REPAIR_NO_VARIANT 0xFFFFFFFFu

typedef struct {               /* one step of one oligo's repair; step 0 is the oligo as it is (72 bytes) */
	pcr_word128 word;          /* the oligo after this step: same slots start..stop, bases only added */
	uint32_t oligo;            /* distinct-oligo id, pcr_pool_products' numbering */
	uint32_t step;
	uint32_t variant;          /* index, in pcr_site_variants' record order for the same arguments, of the variant unioned in; step 0: PCR_REPAIR_NO_VARIANT */
	uint32_t added_mask;       /* bit i: the oligo's slot start+i gained a base in this step; step 0: 0 */
	uint32_t n_expansions;     /* Word::degeneracy() of word */
	uint32_t candidates;       /* candidates weighed for this step; step 0: 0 */
	uint32_t sequences_held, sites_held, variants_held;   /* after this step */
	uint32_t sequences_total;  /* distinct sequences with any site of the oligo at the floor */
	uint32_t gain;             /* sequences_held minus the previous step's; step 0: 0 */
	uint32_t flags;            /* on an oligo's LAST record, why it stopped: one PCR_REPAIR_* reason; 0 on the others */
	uint32_t valid;            /* pcr_thermo's `valid` for word; 0 with args == NULL */
	uint32_t reserved;         /* 0: the record's size is a multiple of 8 either way, this names the last four bytes */
} pcr_repair_step;

/* Which bases to make degenerate to get back the sequences an oligo no longer binds, and what each one buys: a greedy
 * union of observed template spellings into the oligo, one per step, every step reported.
 *   Sites and variants.  Exactly pcr_site_variants' for the same handle state, `which`, panel and threshold: the same
 * picked entry, the same key (flanks included), the same record order -- which does not depend on thermodynamics, so
 * `variant` indexes what pcr_site_variants(args = NULL) returns.  The footprint of a variant is its word at the oligo's
 * slots start..stop; the flanking slots play no part here.
 *   Held.  A word W (the oligo, or the oligo after a step) holds a variant v if at most max_mismatch of the slots k in
 * start..stop have (v[k] & W[k]) == 0 and the clamp3 slots stop-clamp3+1..stop all intersect (clamp3 above the oligo's
 * length: nothing is held).  An empty slot of v is a mismatch; an ambiguity code of the template matches where it
 * intersects (Word::operator&).  For W = the oligo this is popcount(mismatch_mask) <= max_mismatch && v.clamp3 >= clamp3.
 * A sequence is held if any of its sites of this oligo belongs to a held variant.  sequences_held counts distinct
 * sequences, sites_held sums `sites` over the held variants, variants_held counts them.
 *   One step.  Candidates: the first max_candidates variants of the oligo in record order that W does not hold, that
 * carry exactly one base in every footprint slot, and whose union W | footprint(v) has at most max_degeneracy
 * expansions.  Each is weighed by everything its union would hold, not by v alone: gain = sequences held by the union
 * and not by W.  The step takes the highest gain; ties go to the higher sites_held, then the fewer expansions, then the
 * lower variant index.
 *   Stopping.  The oligo's last record carries the reason: every sequence held (COMPLETE); max_steps steps taken
 * (STEPS); no candidate although an unheld single-base variant exists, i.e. every such union exceeds max_degeneracy
 * (DEGENERACY); the best gain is 0 or there is no candidate for another reason (NO_GAIN).  Where several apply:
 * COMPLETE, STEPS, DEGENERACY, NO_GAIN.  An oligo without sites gets its step 0 with zeros and COMPLETE; one that has
 * more than max_degeneracy expansions to begin with stops at step 0 by the same rules.
 *   Thermodynamics.  args != NULL: the words of all steps of all oligos go through pcr_thermo in one batch with
 * check_homo_dimer; `valid` is its verdict.  It is reported, not used as a gate.  args == NULL: valid = 0.
 *   Records are sorted by (oligo, step): max_steps + 1 at most per distinct oligo.  Returns their number or a negative
 * error; if it exceeds cap the contents of out are unspecified (cap = 0: count only, nothing is melted).  n_pairs = 0
 * returns 0.  oligo_id[2*n_pairs] as pcr_site_variants.  The same bytes come out on every run.
 *   PCR_ERR_ARG (checked before the handle): pcr_site_variants' refusals in its order (template_strand taken as 0);
 * max_degeneracy 0 or above PCR_SITE_MAX_EXPANSIONS; clamp3 > 32; max_candidates 0 or above
 * PCR_REPAIR_MAX_CANDIDATES; max_steps above PCR_REPAIR_MAX_STEPS (0 is legal: step 0 only); then a null handle.  The
 * other errors as pcr_site_variants.  Changes nothing other calls read and makes no collective on a sharded handle. */
int64_t pcr_site_repair(pcr_ctx *ctx, pcr_set which, const pcr_pair *pairs, uint32_t n_pairs, float threshold,
	uint32_t max_degeneracy, uint32_t max_mismatch, uint32_t clamp3, uint32_t max_candidates, uint32_t max_steps,
	const pcr_thermo_args *args, int check_homo_dimer, uint32_t *oligo_id, pcr_repair_step *out, uint64_t cap);

/* ---- Every oligo-by-oligo dimer of a primer pool */

/* One cell of the pool's dimer matrix: an ordered pair of distinct-oligo ids, reduced over its duplexes (40 bytes). */
typedef struct {
	uint32_t query_oligo, target_oligo;   /* distinct-oligo ids (as pcr_pool_products); equal: the homodimer cell */
	uint32_t n_duplexes;                  /* D(query) * D(target); homodimer cell: D(query) */
	uint32_t q_expansion, t_expansion;    /* the duplex attaining tm_max, indices in Word::begin()/next() order; homodimer: equal */
	uint32_t flags;                       /* PCR_DIMER_HOMO = 1u */
	float    tm_max, tm_min;              /* highest / lowest Tm over the cell's duplexes, degrees C (NucCruc clamps at 0) */
	float    dH, dS;                      /* of the duplex attaining tm_max */
} pcr_pool_dimer;

#define PCR_DIMER_HOMO 1u
#define PCR_DIMER_RULE_POOL  0   /* pcr_assay.cpp:815-852 */
#define PCR_DIMER_RULE_ASSAY 1   /* pcr_assay.cpp:232-269, valid_pcr.cpp:13 */

/* Which oligos of a pool anneal to each other: the Tm of every ordered pair of the pool's distinct oligos, and of every oligo
 * with itself.
 *   Oligo ids.  The pool's 2*n_pool oligo words get distinct ids in order of first appearance, as in pcr_pool_products;
 * oligo_id[2*n_pool] receives them.  D(x) = Word::degeneracy() of oligo x.
 *   Cells.  There is a cell for every ordered pair (q, t), 0 <= q, t < n_distinct, in row-major order.  The order matters:
 * NucCruc::approximate_tm_heterodimer is not symmetric under exchange of query and target (the last bits of Tm, dH and dS
 * differ for most pairs), so the result is a full matrix, not a triangle.  Off the diagonal the cell's duplexes are
 * (expansion iq of q) x (expansion it of t), expansions in the order of Word::begin() / next(), duplex iq * D(t) + it (the
 * reference's loops, query outer), each NucCruc::approximate_tm_heterodimer with query = q's expansion and target = t's
 * expansion, both spelt 5'->3' as the words hold them.  On the diagonal there is one duplex per expansion,
 * NucCruc::approximate_tm_homodimer of that expansion, as PCR::is_valid loops (valid_pcr.cpp:34-41); the homodimer is not
 * the heterodimer of an oligo with itself (the symmetry term changes dS).  Dimers between DIFFERENT expansions of one
 * degenerate oligo are not formed: the diagonal cell has D(q) duplexes, not D(q)^2.
 *   Strand concentration, salt = args->salt (only salt and primer_strand of args are read).  PCR_DIMER_RULE_POOL: every
 * duplex at args->primer_strand, no degeneracy correction -- with it, the maximum of tm_max over the four cells
 * (a.F, a.R) x (b.F, b.R) decides pcr_multiplex_compatible(a, b) exactly (incompatible iff that maximum >= max_dimer).
 * PCR_DIMER_RULE_ASSAY: off the diagonal NucCruc's two-concentration rule (nuc_cruc.h:818-838) of primer_strand / D(q) and
 * primer_strand / D(t) -- with it, tm_max of cell (F, R) is pcr_dimer of the assay (F, R); on the diagonal
 * primer_strand / D(q), PCR::is_valid's (valid_pcr.cpp:13).
 *   Reduction.  tm_max and tm_min are taken over the cell's duplexes; q_expansion, t_expansion, dH and dS are those of the
 * duplex attaining tm_max, the lowest-numbered one on a tie (ties are common: most random pairs melt below 0 C and are
 * clamped to Tm 0 with different dH).
 *   Records are the cells with tm_max >= tm_floor, in cell order; tm_floor <= 0 keeps all n_distinct^2 cells.  Returns their
 * number or a negative error; if it exceeds cap the contents of out are unspecified (cap = 0: count only; with tm_floor > 0
 * that still runs the thermodynamics).  n_pool = 0 returns 0.
 *   PCR_ERR_ARG (from the arguments alone, checked before the handle, in this order): null pointers or cap without out;
 * n_pool > PCR_POOL_MAX_PAIRS; an unknown rule; primer_strand <= 0; salt outside [1e-6, 1]; an oligo that is empty, has a
 * hole between its ends or more than PCR_SITE_MAX_EXPANSIONS expansions (which keeps every cell within the 65 536 duplexes
 * of pcr_dimer).  PCR_ERR_CAPACITY (also before the handle) when the pool's duplexes number 2^31 or more.  Then a null
 * handle.  PCR_ERR_RANGE if a trace-back fails inside the engine.
 *   Needs no sequence set and no word DB: it runs on a fresh handle, changes nothing other calls read, and is the same on a
 * handle with a target shard attached (no collective is made). */
int64_t pcr_pool_dimers(pcr_ctx *ctx, const pcr_pair *pool, uint32_t n_pool, const pcr_thermo_args *args, int rule,
	float tm_floor, uint32_t *oligo_id, pcr_pool_dimer *out, uint64_t cap);

/* ---- Which oligos of a pool extend on each other: 3'-anchored dimers */

/* One qualifying placement of a duplex: the query's 3' end paired on the target, with template to copy (40 bytes). */
typedef struct {
	uint32_t query_oligo, target_oligo;   /* distinct-oligo ids (as pcr_pool_dimers); equal: the oligo on a second copy of itself */
	uint32_t q_expansion, t_expansion;    /* the duplex, indices in Word::begin()/next() order; on the diagonal: equal */
	uint8_t  run, extension;              /* Watson-Crick pairs from the query's 3' base on; target bases 5' of the paired end (= the placement j) */
	uint8_t  overlap, overlap_matches;    /* positions where the strands face each other; the Watson-Crick pairs among them */
	uint32_t flags;                       /* PCR_DIMER_HOMO, PCR_DIMER_END3_MUTUAL */
	float    dG, tm, dH, dS;              /* of the run alone as a heterodimer; dG = dH - 310.15 * dS in float (kcal/mol), tm in degrees C */
} pcr_dimer_placement;

/* One cell of the pool's 3'-anchored dimer matrix, reduced over its qualifying placements (48 bytes). */
typedef struct {
	uint32_t query_oligo, target_oligo;   /* as pcr_pool_dimer */
	uint32_t n_duplexes;                  /* D(query) * D(target); on the diagonal D(query) */
	uint32_t n_placements;                /* qualifying placements over all duplexes of the cell, before the dG filter */
	uint32_t q_expansion, t_expansion;    /* the best placement's duplex */
	uint8_t  run, extension, overlap, overlap_matches;   /* the best placement's */
	uint32_t flags;                       /* PCR_DIMER_HOMO; PCR_DIMER_END3_MUTUAL of the best placement */
	float    dG, tm, dH, dS;              /* the best placement's */
} pcr_pool_dimer_end3;

#define PCR_DIMER_END3_MUTUAL 2u   /* the run reaches the target's 3' end: both oligos extend */

/* Which oligos of a pool extend on each other (Primer3's "end" complementarity, with the engine's energies).  pcr_pool_dimers
 * melts the best duplex of two whole oligos and does not say where it sits; a primer-dimer artefact needs less and something
 * else: a few clean base pairs at a 3' end and, beyond it, template for the polymerase to copy.
 *   Oligo ids, cells and duplexes are pcr_pool_dimers': ids in order of first appearance (oligo_id[2*n_pool] receives them), a
 * cell per ordered (query q, target t), off the diagonal D(q)*D(t) duplexes, duplex iq * D(t) + it (query expansion outer).
 * On the diagonal the cell has D(q) duplexes: expansion x against a second copy of x, the oligo priming on its own kind.
 *   Placements.  Both strands are spelt 5'->3' as the words hold them, x with Lx bases, y with Ly.  Placement j, 0 <= j < Ly,
 * puts x's 3' base opposite y[j], antiparallel: x[Lx-1-k] faces y[j+k] for 0 <= k < overlap = min(Lx, Ly - j).  run = the
 * number of consecutive Watson-Crick pairs (A.T and C.G only) counted from k = 0; overlap_matches = the Watson-Crick pairs
 * among all overlap positions; extension = j, the bases of y 5' of the paired end, which the polymerase copies: the product
 * is x + revcomp(y[0 .. j-1]).  A placement qualifies if run >= min_run and extension >= min_extension.
 * PCR_DIMER_END3_MUTUAL is set where j + run == Ly: the run reaches y's 3' end and both oligos extend.  Corner cases: the run
 * never exceeds the overlap, so oligos shorter than min_run have no placement; j = 0 has nothing to copy and qualifies only
 * with min_extension = 0; a run of the whole query (run == Lx) is legal; on the diagonal, a palindromic 3' end of r bases
 * gives run >= r at j = Lx - r, which is MUTUAL.
 *   Melt.  Every qualifying placement is melted as the heterodimer of the run alone: NucCruc::approximate_tm_heterodimer with
 * query = x's last `run` bases and target = y[j .. j+run-1], on the diagonal too.  Salt and strand concentration are
 * pcr_pool_dimers' `rule` for cell (q, t) off the diagonal; on the diagonal the same off-diagonal rule with t = q (under
 * PCR_DIMER_RULE_ASSAY half of primer_strand / D(q)).  It yields tm, dH and dS; dG = dH - 310.15f * dS in float, as
 * pcr_thermo_result.dG.  The engine gives all zeros to perfect duplexes of 1 and 2 bases and energies from 3 bases on, so
 * min_run is 3 .. 32; min_extension is 0 .. 31.
 *   Placement records (place_out): in cell order, then duplex order, then j ascending; kept where the placement's own
 * dG <= dg_max (+INFINITY keeps all).
 *   Cell records (out): the cells with at least one kept placement, in cell order.  n_placements counts the qualifying
 * placements before the dG filter.  The best placement has the lowest dG; on a tie the longer run, then the lower duplex
 * number, then the lower j (ties are common: the same 3-mer duplex at two places of a target gives identical floats).  Its
 * expansions, its four byte fields, its four floats and its MUTUAL flag are the cell's.
 *   Returns the number of cell records or a negative error; *n_place, if not NULL, receives the number of placement
 * records.  Past cap the contents of out are unspecified, past place_cap those of place_out; cap = 0 and place_cap = 0
 * count only, and with dg_max = +INFINITY such a count call runs no thermodynamics.  n_pool = 0 returns 0.
 *   PCR_ERR_ARG (from the arguments alone, checked before the handle, in this order): null pointers, cap without out or
 * place_cap without place_out; n_pool > PCR_POOL_MAX_PAIRS; an unknown rule; primer_strand <= 0; salt outside [1e-6, 1];
 * min_run outside 3 .. 32; min_extension above 31; dg_max NaN; then the oligos as pcr_pool_dimers (empty, a hole, too many
 * expansions).  PCR_ERR_CAPACITY as pcr_pool_dimers.  Then a null handle.  PCR_ERR_RANGE if a trace-back fails.
 *   Needs no sequence set and no word DB, changes nothing other calls read, makes no collective on a sharded handle.
 *   Out of scope: anchors with gaps or bulges, or a mismatch inside the run; hairpin self-priming of a single strand;
 * treating probes (3'-blocked oligos) differently.  pcr_pool_conflicts_ext reduces these cells to pairs of pool rows. */
int64_t pcr_pool_dimers_end3(pcr_ctx *ctx, const pcr_pair *pool, uint32_t n_pool, const pcr_thermo_args *args, int rule,
	uint32_t min_run, uint32_t min_extension, float dg_max, uint32_t *oligo_id,
	pcr_pool_dimer_end3 *out, uint64_t cap, pcr_dimer_placement *place_out, uint64_t place_cap, uint64_t *n_place);

/* ---- Products of a pool with the Tm of their two sites, Tm-floored, and the pool's amplification bitsets at that floor */

/* One product with the duplex Tm of its plus site and of its minus site (48 bytes). */
typedef struct {
	uint32_t plus_oligo, minus_oligo, sequence;
	int32_t  begin, end, inner_start, inner_length;
	uint32_t intended;                  /* the eight fields of pcr_product, same meaning */
	float    tm_plus, tm_minus;         /* tm_max of the plus site / of the minus site, degrees C */
	uint32_t flags;                     /* PCR_PRODUCT_* */
	uint32_t reserved;                  /* 0 */
} pcr_product_tm;

#define PCR_PRODUCT_PLUS_NO_TM  1u      /* the plus site is a PCR_SITE_NO_TM site: tm_plus = 0 */
#define PCR_PRODUCT_MINUS_NO_TM 2u      /* the same for the minus site and tm_minus */

/* Which products of a pool form at an annealing temperature, and which sequences each pool pair still amplifies there: the
 * records of pcr_pool_products joined on the device with the site Tm of pcr_site_tm, floored, and reduced to bitsets.
 *   Products.  Exactly the records pcr_pool_products returns for the same handle state, pool, threshold and amplicon range:
 * the same eight fields, uniqueness and order by (plus_oligo, minus_oligo, sequence, begin, end); oligo_id[2*n_pool] is the
 * same numbering.  That is: a product joins a plus site (strand 1) of oligo x with a minus site (strand 2) of oligo y on one
 * sequence, with p3 < m5 (loc3 of the plus site before loc5 of the minus site), amp_min <= m3 - p5 + 1 <= amp_max, the
 * inner stretch (inner_start = p3 - 3, inner_length = m5 - inner_start + 8, as pcr_amplicon) inside the sequence and free
 * of EOS; begin = p5, end = m3.
 *   Tm.  tm_plus is tm_max of the record pcr_site_tm returns for (plus_oligo, sequence, loc5 = begin, strand 1) with the same
 * args and template_strand, tm_minus that of (minus_oligo, sequence, loc3 = end, strand 2) -- bit for bit: the entry the
 * target is read from, PCR_SITE_NO_TM, the lowest expansion winning a tie and the two-concentration rule are pcr_site_tm's.
 * A PCR_SITE_NO_TM site gives Tm 0 and its bit in flags.
 *   Floor.  A product is kept iff tm_floor <= 0 or min(tm_plus, tm_minus) >= tm_floor (in float).  Records are the kept
 * products, in order.  Returns their number or a negative error; if it exceeds cap the contents of out are unspecified
 * (cap = 0: count only).  n_pool = 0 returns 0.
 *   Bitsets.  bits_fr / bits_rf, either may be NULL: n_pool x pcr_bitset_words(ctx, which) u64 in the bit layout of
 * pcr_amplify.  Bit s of row i of bits_fr is set iff a kept product has plus_oligo = id(F_i), minus_oligo = id(R_i) and
 * sequence s; bits_rf the same with plus_oligo = id(R_i), minus_oligo = id(F_i).  Rows are written in full, zeros included,
 * whenever the call returns >= 0 -- also when the count exceeds cap and with cap = 0; they are reduced on the device from the
 * join, not from the records.  Pool pairs with the same (F, R) get equal rows; a pair with F = R gets bits_fr = bits_rf.
 *   The thermodynamics run iff tm_floor > 0, records are written (cap > 0) or a bitset is asked for; otherwise the call is
 * pcr_pool_products' count.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in pcr_site_tm's order: unknown set or PCR_SET_MULTIPLEX;
 * null pointers or cap without out; n_pool > PCR_POOL_MAX_PAIRS; a negative concentration; salt outside [1e-6, 1]; an oligo
 * that is empty, has a hole between its ends, more than PCR_SITE_MAX_EXPANSIONS expansions or a zero strand concentration;
 * then a tm_floor that is not finite; then a null handle.  PCR_ERR_STATE without a word DB; PCR_ERR_CAPACITY for 2^31 or
 * more sites, (site, expansion) jobs or products; PCR_ERR_RANGE if a trace-back fails inside the engine.  Changes nothing
 * other calls read.  On a handle with a target shard attached, sequence indices are local to the rank's block and no
 * collective is made (as pcr_pool_products). */
int64_t pcr_pool_products_tm(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	uint32_t *oligo_id, pcr_product_tm *out, uint64_t cap, uint64_t *bits_fr, uint64_t *bits_rf);

/* ---- Products of a pool under a 3'-end extension rule */

/* What a product's two sites must show at the 3' end of their primers, the end the polymerase extends from. */
typedef struct {
	uint32_t min_clamp3;                /* 0 = off */
	uint32_t window;                    /* 0 .. 32: how many slots at the 3' end max_end_mismatch looks at */
	uint32_t max_end_mismatch;          /* mismatching slots allowed inside the window */
	int32_t  use_taq_mama;              /* 0 / 1: id_plus / id_minus carry update_identity's TaqMAMA factor */
	float    ident_threshold;           /* 0 = off; else keep iff sqrtf(id_plus * id_minus) >= ident_threshold */
} pcr_end3_rule;

/* One product with the Tm and the 3' end of its plus site and of its minus site (64 bytes). */
typedef struct {
	uint32_t plus_oligo, minus_oligo, sequence;
	int32_t  begin, end, inner_start, inner_length;
	uint32_t intended;
	float    tm_plus, tm_minus;
	uint32_t flags;                     /* PCR_PRODUCT_* */
	uint32_t reserved;                  /* 0; the twelve fields of pcr_product_tm, same meaning, same bytes (48) */
	uint8_t  clamp3_plus, clamp3_minus; /* consecutive matching slots from the oligo's last slot downwards */
	uint8_t  end_mismatch_plus, end_mismatch_minus;   /* mismatching slots among the last min(window, length) */
	float    id_plus, id_minus;         /* update_identity's score of the oligo at the site */
	uint32_t reserved2;                 /* 0 */
} pcr_product_end3;

/* pcr_pool_products_tm with a rule on where the mismatches of the two sites lie: a site whose only mismatch is under the
 * primer's last base melts a degree or two below the exact site and is the textbook site that does not extend.
 *   Products, Tm, floor, order, bitsets, oligo_id.  Exactly pcr_pool_products_tm's for the same handle state and arguments.
 * args may be NULL: no thermodynamics run, both Tm are 0 and flags is 0; tm_floor > 0 is then refused, and no concentration
 * or salt is looked at (as pcr_site_variants without args).
 *   Per-site quantities.  Taken from the entry pcr_site_tm reads the site from (among the entries sharing the site's loc and
 * strand and matching the oligo, the one with the most occupied slots in the oligo's window; on a tie the lowest slot masks),
 * so they agree with the site's pcr_site_variants record.  For oligo c with slots start .. stop and that entry's word w, slot k
 * matches iff c and w share a base there (Word & Word per slot); an empty slot of w -- a site hanging over a sequence end --
 * is a mismatch.  clamp3: the consecutive matching slots from stop downwards (= pcr_site_variant.clamp3).  end_mismatch: the
 * mismatching slots among the last min(window, length) slots, 0 with window = 0.  id: (float)matches * float(1.0/length) in
 * float, matches as pcr_site.matches; with use_taq_mama times update_identity's factor (optimize.cpp:209-261), min(1,
 * c_taq_mama[template's last two][primer's last two]), in float, applied only when the oligo's last two slots and the word's
 * two slots under them each hold exactly one base.  That is the score pcr_amplify tests for the same oligo and word.
 *   Rule.  A product that passes the Tm floor is kept iff for both sites clamp3 >= min(min_clamp3, length) and, with window >
 * 0, end_mismatch <= max_end_mismatch; and ident_threshold == 0 or sqrtf(id_plus * id_minus) >= ident_threshold (product and
 * root in float, correctly rounded: pcr_amplify's test).  rule = NULL or an all-zero rule keeps everything: the first 48
 * bytes of every record are then pcr_pool_products_tm's record and the bitsets are its bitsets.  Records, the return value
 * and the bitsets are of the kept products; *n_before_rule (may be NULL) receives the number past the Tm floor before the
 * rule.  cap, out, bits_fr / bits_rf and the condition under which the thermodynamics run (with args) are
 * pcr_pool_products_tm's: cap = 0 counts, a count above cap leaves out unspecified, rows are written in full whenever the
 * call returns >= 0 and are reduced on the device from the join.
 *   PCR_ERR_ARG, from the arguments alone and before the handle: pcr_pool_products_tm's checks in its order, the
 * concentration and salt ones only with args; after the tm_floor that is not finite: window, min_clamp3 or max_end_mismatch
 * above 32; use_taq_mama neither 0 nor 1; ident_threshold not finite or outside [0, 1]; tm_floor > 0 without args; then a
 * null handle.  PCR_ERR_STATE, PCR_ERR_CAPACITY (also for 2^31 or more products before the rule) and PCR_ERR_RANGE as
 * pcr_pool_products_tm.  Changes nothing other calls read.  On a handle with a target shard attached, sequence indices are
 * local to the rank's block and no collective is made.  pcr_pool_anneal_profile_end3, pcr_pool_conflicts_end3 and
 * pcr_pool_probe_hits_end3 apply the same rule inside their joins. */
int64_t pcr_pool_products_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args /* may be NULL */, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, uint32_t *oligo_id, pcr_product_end3 *out, uint64_t cap,
	uint64_t *bits_fr, uint64_t *bits_rf, uint64_t *n_before_rule /* may be NULL */);

/* ---- Annealing profile: what a pool amplifies at every temperature of a gradient, from one melt and one join */

#define PCR_ANNEAL_MAX_TEMPS 256
#define PCR_ANNEAL_NO_PRODUCT (-1.0f)     /* melt value of a cell / sequence without any product */

typedef struct {                          /* one temperature of the profile (40 bytes) */
	float    temperature;                 /* temps[t], as given */
	uint32_t reserved;                    /* 0 */
	uint64_t products_intended;           /* products kept at this floor with pcr_product.intended = 1 */
	uint64_t products_spurious;           /* ... with intended = 0 */
	uint64_t cells;                       /* sum over pool rows i of pair_sequences[i][t] */
	uint64_t spurious_sequences;          /* sequences that carry at least one kept spurious product */
} pcr_anneal_point;

/* Which products of a pool form, and which sequences each pool pair amplifies, at every temperature of an ascending list:
 * what n_temps calls of pcr_pool_products_tm with tm_floor = temps[t] answer, from one melt of the sites and one join.
 *   Products.  Exactly the products pcr_pool_products_tm forms for the same handle state, pool, threshold, amplicon range,
 * args and template_strand with no floor; oligo_id[2*n_pool] is the same numbering.  A product's melt value is
 * v = min(tm_plus, tm_minus), both Tm bit for bit those of pcr_pool_products_tm (a PCR_SITE_NO_TM site gives 0).
 *   Keeping rule (pcr_pool_products_tm's, restated).  A product is kept at temps[t] iff !(temps[t] > 0) || v >= temps[t],
 * in float.
 *   Melt matrices.  melt_fr / melt_rf, either may be NULL: n_pool x pcr_num_sequences(ctx, which) floats, row-major.
 * melt_fr[i][s] is the maximum of v over the products with plus_oligo = id(F_i), minus_oligo = id(R_i) and sequence s,
 * melt_rf[i][s] the same with the two oligos exchanged; PCR_ANNEAL_NO_PRODUCT where the cell has no product, +0.0f where its
 * only products have v = 0.  For every finite floor f, bit s of row i of bits_fr of pcr_pool_products_tm at tm_floor = f
 * is set iff melt_fr[i][s] >= 0 && (!(f > 0) || melt_fr[i][s] >= f), and likewise melt_rf and bits_rf.  Pool pairs with the
 * same (F, R) get equal rows; a pair with F = R gets melt_fr = melt_rf.  melt_spurious, may be NULL:
 * pcr_num_sequences(ctx, which) floats, the maximum of v over the products on s with intended = 0 ({plus, minus} is no pool
 * pair in either orientation), PCR_ANNEAL_NO_PRODUCT where there is none.  Everything asked for is written in full whenever
 * the call returns >= 0.  The maxima are reduced on the device with integer atomics on the floats' bit patterns (v >= +0):
 * the bytes do not depend on the order the device works in.
 *   Points.  points[t], n_temps records: products_intended + products_spurious is what pcr_pool_products_tm returns with
 * tm_floor = temps[t] and cap = 0.  pair_sequences, may be NULL: n_pool x n_temps, row-major; pair_sequences[i][t] is the
 * number of sequences s whose max(melt_fr[i][s], melt_rf[i][s]) is a product's and is kept at temps[t] -- the population of
 * bits_fr[i] | bits_rf[i] at that floor.  cells sums it over the pool rows (a repeated pair counts again) and is written
 * also without pair_sequences; spurious_sequences counts the sequences whose melt_spurious is kept at temps[t].
 *   Returns the number of products with no floor (pcr_pool_products' count) or a negative error.  n_pool = 0 returns 0 and
 * writes points with zero counts and the temperatures.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in pcr_pool_products_tm's order: unknown set or
 * PCR_SET_MULTIPLEX; a null args, temps or points, or a null pool or oligo_id with n_pool > 0; n_pool > PCR_POOL_MAX_PAIRS;
 * a negative concentration; salt outside [1e-6, 1]; an oligo that is empty, has a hole between its ends, more than
 * PCR_SITE_MAX_EXPANSIONS expansions or a zero strand concentration; then n_temps = 0 or n_temps > PCR_ANNEAL_MAX_TEMPS;
 * then a temperature that is not finite or temps not strictly ascending; then a null handle.  PCR_ERR_STATE without a word
 * DB; PCR_ERR_CAPACITY for 2^31 or more sites, (site, expansion) jobs or products, or when the melt rows of the pool's
 * distinct (F, R) would not fit in free device memory; PCR_ERR_RANGE if a trace-back fails inside the engine.  Changes
 * nothing other calls read.  The number of kernel launches and copies does not depend on n_temps.  On a handle with a
 * target shard attached, sequence indices are local to the rank's block and no collective is made. */
int64_t pcr_pool_anneal_profile(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand,
	const float *temps, uint32_t n_temps, uint32_t *oligo_id,
	pcr_anneal_point *points,             /* n_temps */
	uint32_t *pair_sequences,             /* n_pool x n_temps, row-major; may be NULL */
	float *melt_fr, float *melt_rf,       /* n_pool x pcr_num_sequences(ctx, which) each; either may be NULL */
	float *melt_spurious);                /* pcr_num_sequences(ctx, which); may be NULL */

/* pcr_pool_anneal_profile over the products that pass a 3'-end rule: the product set is the one pcr_pool_products_end3 keeps
 * for the same handle state, pool, threshold, amplicon range, args, template_strand and rule.
 *   Rule.  The per-site quantities (clamp3, end_mismatch over the last min(window, length) slots, the identity score with or
 * without the TaqMAMA factor) and the test (both sites, then ident_threshold == 0 or sqrtf(id_plus * id_minus) >=
 * ident_threshold) are pcr_pool_products_end3's.  The rule does not depend on temperature: a product that fails it is absent
 * from points, pair_sequences, cells, spurious_sequences and the three melt matrices at every temperature, and its cell stays
 * PCR_ANNEAL_NO_PRODUCT unless another product fills it.  For every finite T, the rows of melt_fr / melt_rf with value >= T
 * (all rows with a product where T <= 0) are bits_fr / bits_rf of pcr_pool_products_end3 at tm_floor = T with the same rule.
 *   Returns the number of products that pass the rule with no floor, or a negative error.  rule = NULL or an all-zero rule:
 * every output buffer and the return value are pcr_pool_anneal_profile's, byte for byte, and nothing is computed per site.
 * args stays mandatory.
 *   PCR_ERR_ARG, from the arguments alone and before the handle: pcr_pool_anneal_profile's checks in its order; then window,
 * min_clamp3 or max_end_mismatch above 32; use_taq_mama neither 0 nor 1; ident_threshold not finite or outside [0, 1]; then a
 * null handle.  PCR_ERR_STATE, PCR_ERR_CAPACITY and PCR_ERR_RANGE as pcr_pool_anneal_profile.  Changes nothing other calls
 * read.  On a handle with a target shard attached, sequence indices are local to the rank's block and no collective is made. */
int64_t pcr_pool_anneal_profile_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, const pcr_end3_rule *rule,
	const float *temps, uint32_t n_temps, uint32_t *oligo_id, pcr_anneal_point *points, uint32_t *pair_sequences,
	float *melt_fr, float *melt_rf, float *melt_spurious);

/* ---- Pool conflicts: which assays of a pool cannot share a tube */

typedef struct {                          /* one unordered pair of pool rows (48 bytes) */
	uint32_t row_a, row_b;                /* pool rows, row_a <= row_b; equal: the assay against itself */
	uint64_t products;                    /* spurious products attributed to the cell and kept at tm_floor */
	uint32_t sequences;                   /* distinct `sequence` values among them */
	float    melt;                        /* max of v = min(tm_plus, tm_minus) over them; PCR_ANNEAL_NO_PRODUCT if products = 0 */
	uint32_t melt_sequence;               /* the lowest sequence among the products attaining melt; 0 if products = 0 */
	float    dimer_tm;                    /* max tm_max over the cell's dimer cells; 0 when dimers are not asked for */
	uint32_t dimer_query, dimer_target;   /* distinct-oligo ids of the dimer cell attaining it, lowest (q, t) on a tie; 0, 0 without dimers */
	uint32_t flags;                       /* PCR_CONFLICT_PRODUCT: products > 0; PCR_CONFLICT_DIMER: dimers asked for and dimer_tm >= dimer_floor */
	uint32_t reserved;                    /* 0 */
} pcr_pool_conflict;

#define PCR_CONFLICT_PRODUCT 1u
#define PCR_CONFLICT_DIMER   2u
#define PCR_CONFLICT_NO_DIMERS (-1)       /* dimer_rule: run no dimer thermodynamics */

/* Which pairs of assays (pool rows) of a pool conflict: pcr_pool_products_tm's spurious products and pcr_pool_dimers' cells,
 * reduced on the device to the unordered pairs of pool rows.  No reference counterpart beyond multiplex_compatible.
 *   Products.  Exactly the products pcr_pool_products_tm forms for the same handle state, pool, threshold, amplicon range,
 * args, template_strand and tm_floor: the same oligo numbering (oligo_id[2*n_pool]), tm_plus and tm_minus bit for bit, the
 * same keeping rule !(tm_floor > 0) || v >= tm_floor with v = min(tm_plus, tm_minus) + 0.0f (no -0 appears).  Only products
 * with intended = 0 take part.
 *   Attribution.  O(i) = {id(F_i), id(R_i)}.  A spurious product with plus oligo x and minus oligo y belongs to the set of
 * unordered row pairs {i, j}, i = j allowed, with (x in O(i) and y in O(j)) or (x in O(j) and y in O(i)), and counts once in
 * each cell of that set however many ways the cell arises.  Repeated and exchanged pool rows are separate rows: an F-F
 * product of a primer shared by rows i and j belongs to {i,i}, {i,j} and {j,j}, once each.
 *   Dimers.  Only with dimer_rule = PCR_DIMER_RULE_POOL or PCR_DIMER_RULE_ASSAY.  The dimer cells of {a, b} are the ordered
 * pcr_pool_dimers cells (q, t) with (q in O(a), t in O(b)) or (q in O(b), t in O(a)), the homodimer cell where q = t, out
 * of the full matrix of pcr_pool_dimers for the same pool, args and rule with tm_floor = 0, bit for bit; dimer_tm is the
 * highest tm_max among them.  With PCR_DIMER_RULE_POOL, pcr_multiplex_compatible(a, b) and (b, a) both hold iff
 * dimer_tm < max_dimer.  With PCR_CONFLICT_NO_DIMERS no dimer thermodynamics run, the three dimer fields are 0 and nothing
 * pcr_pool_dimers alone asks for is needed.
 *   Records.  One for every cell with products > 0 and, with a dimer rule, for every cell with dimer_tm >= dimer_floor
 * (dimer_floor <= 0: all n_pool(n_pool + 1)/2 cells), sorted by (row_a, row_b).  The reduction is a sort by (cell, sequence)
 * and a segmented reduction over integers: the bytes do not depend on the order the device works in.
 *   Returns the number of records or a negative error; if it exceeds cap the contents of out are unspecified (cap = 0:
 * count only).  n_pool = 0 returns 0.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in pcr_pool_products_tm's order (unknown set or
 * PCR_SET_MULTIPLEX; null pointers or cap without out; n_pool > PCR_POOL_MAX_PAIRS; a negative concentration; salt outside
 * [1e-6, 1]; an oligo that is empty, has a hole between its ends, more than PCR_SITE_MAX_EXPANSIONS expansions or a zero
 * strand concentration; a tm_floor that is not finite); then a dimer_rule that is none of the three values; then a
 * dimer_floor that is not finite; then, with a dimer rule, primer_strand <= 0 or primer_strand / degeneracy underflowing to
 * zero (pcr_pool_dimers' refusals); then a null handle.  PCR_ERR_STATE without a word DB, also when only dimers would
 * produce records: the call is about a pool on a set.  PCR_ERR_CAPACITY for 2^31 or more sites, (site, expansion) jobs or
 * (product, cell) attributions, and with a dimer rule for 2^31 or more duplexes; PCR_ERR_RANGE if a trace-back fails inside
 * the engine.  Changes nothing other calls read.  On a handle with a target shard attached, sequence indices are local to
 * the rank's block and no collective is made. */
int64_t pcr_pool_conflicts(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	int dimer_rule, float dimer_floor, uint32_t *oligo_id, pcr_pool_conflict *out, uint64_t cap);

/* pcr_pool_conflicts over the products that pass a 3'-end rule: the products that take part are the spurious ones
 * pcr_pool_products_end3 keeps for the same handle state, pool, threshold, amplicon range, args, template_strand, tm_floor
 * and rule (its per-site quantities and its test, after the floor).  Only those are attributed; products, sequences, melt,
 * melt_sequence and PCR_CONFLICT_PRODUCT follow from them, so two allele-specific assays whose only cross product cannot be
 * extended no longer conflict.  The dimer half is untouched: dimer_tm, dimer_query, dimer_target and PCR_CONFLICT_DIMER are
 * pcr_pool_conflicts' for the same arguments, and so is which cells a dimer rule keeps.
 *   Returns the number of records or a negative error; cap and out as pcr_pool_conflicts.  rule = NULL or an all-zero rule:
 * out and the return value are pcr_pool_conflicts', byte for byte, and nothing is computed per site.  args stays mandatory.
 *   PCR_ERR_ARG, from the arguments alone and before the handle: pcr_pool_conflicts' checks in its order, the dimer ones
 * included; then window, min_clamp3 or max_end_mismatch above 32; use_taq_mama neither 0 nor 1; ident_threshold not finite or
 * outside [0, 1]; then a null handle.  PCR_ERR_STATE, PCR_ERR_CAPACITY and PCR_ERR_RANGE as pcr_pool_conflicts.  Changes
 * nothing other calls read.  On a handle with a target shard attached, sequence indices are local to the rank's block and no
 * collective is made. */
int64_t pcr_pool_conflicts_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, int dimer_rule, float dimer_floor, uint32_t *oligo_id, pcr_pool_conflict *out, uint64_t cap);

typedef struct {            /* how pcr_pool_conflicts_ext looks for extensible dimers; NULL = it does not */
	int32_t  rule;          /* PCR_DIMER_RULE_POOL / PCR_DIMER_RULE_ASSAY: pcr_pool_dimers_end3's strand-concentration rule */
	uint32_t min_run;       /* 3 .. 32 */
	uint32_t min_extension; /* 0 .. 31 */
	float    dg_max;        /* +INFINITY keeps every qualifying placement; NaN refused */
} pcr_dimer_end3_args;

typedef struct {            /* one unordered pair of pool rows (96 bytes) */
	pcr_pool_conflict c;                              /* as pcr_pool_conflicts_end3 computes it; PCR_CONFLICT_EXTENSION added to c.flags */
	uint32_t ext_cells;                               /* distinct ordered dimer cells of {a, b} with at least one kept placement (dG <= dg_max) */
	uint32_t ext_placements;                          /* n_placements summed over the distinct dimer cells of {a, b}, before the dG filter */
	uint32_t ext_query, ext_target;                   /* the ordered cell (q, t) that holds the best placement */
	uint32_t ext_q_expansion, ext_t_expansion;        /* the best placement's duplex ... */
	uint8_t  ext_run, ext_extension, ext_overlap, ext_overlap_matches;   /* ... its geometry ... */
	uint32_t ext_flags;                               /* ... PCR_DIMER_HOMO, PCR_DIMER_END3_MUTUAL ... */
	float    ext_dG, ext_tm, ext_dH, ext_dS;          /* ... and energies: that cell's pcr_pool_dimer_end3 record */
} pcr_pool_conflict_ext;

#define PCR_CONFLICT_EXTENSION 4u   /* in c.flags: ext_cells > 0 */

/* pcr_pool_conflicts_end3 with a third half: the 3'-extensible dimers of pcr_pool_dimers_end3, reduced on the device to the
 * unordered pairs of pool rows.  dimer_tm says how well two whole oligos stick; the extension half says whether a polymerase
 * can copy one oligo off the other, which is what makes a primer-dimer artefact.
 *   Base half.  c is what pcr_pool_conflicts_end3 computes for the same handle state, pool, threshold, amplicon range, args,
 * template_strand, tm_floor, rule, dimer_rule and dimer_floor, byte for byte, also in a cell that call would not have kept
 * (its products, melt and dimer fields are computed all the same; PCR_CONFLICT_DIMER is tested against dimer_floor).
 * PCR_CONFLICT_EXTENSION is OR-ed into c.flags afterwards.
 *   Extension half.  Only with ext != NULL.  The dimer cells of {a, b} are pcr_pool_conflicts': the ordered (q, t) with
 * (q in O(a), t in O(b)) or (q in O(b), t in O(a)).  That list of up to eight has repeats when a = b, when a row has F = R
 * or when the rows share an oligo; every distinct ordered cell counts once.  For each, take the cell record of
 * pcr_pool_dimers_end3(pool, args, ext->rule, ext->min_run, ext->min_extension, ext->dg_max), bit for bit.  ext_placements
 * is the sum of their n_placements (before the dG filter); ext_cells is the number of them that call keeps (at least one
 * placement with dG <= dg_max).  The best placement of {a, b} is the best of the kept cells' best placements: the lowest
 * dG, then the longer run, then the lowest (q, t).  The fields ext_query .. ext_dS are that cell record's; with
 * ext_cells = 0 they are all zero, and ext_placements may still be positive (every placement failed dg_max).  No placement
 * records are listed.  dimer_rule and ext are independent: PCR_CONFLICT_NO_DIMERS with ext set runs no whole-oligo
 * thermodynamics, and ext->rule need not be dimer_rule.
 *   Records.  One for every cell pcr_pool_conflicts_end3 keeps and for every cell with ext_cells > 0, sorted by
 * (row_a, row_b).  With ext = NULL the record set and every c are pcr_pool_conflicts_end3's, byte for byte, and all ext
 * fields are zero.  Each cell is reduced by one thread that walks its distinct dimer cells in (q, t) order: no atomics, the
 * bytes do not depend on the order the device works in.
 *   Returns the number of records or a negative error; if it exceeds cap the contents of out are unspecified (cap = 0:
 * count only).  n_pool = 0 returns 0.
 *   PCR_ERR_ARG, from the arguments alone and before the handle: pcr_pool_conflicts_end3's checks in its order; then, with
 * ext set: an ext->rule that is neither PCR_DIMER_RULE_POOL nor PCR_DIMER_RULE_ASSAY; min_run outside 3 .. 32;
 * min_extension above 31; dg_max NaN; primer_strand <= 0 or primer_strand / degeneracy underflowing to zero under
 * ext->rule; then a null handle.  PCR_ERR_STATE without a word DB, also when only the extension half would produce
 * records.  PCR_ERR_CAPACITY as pcr_pool_conflicts_end3, and with ext set for 2^31 or more duplexes; PCR_ERR_RANGE if a
 * trace-back fails inside the engine.  The dense matrix of cell records takes 48 bytes per ordered pair of distinct oligos
 * on the device.  Changes nothing other calls read.  On a handle with a target shard attached, sequence
 * indices are local to the rank's block and no collective is made.
 *   Out of scope: probes as 3'-blocked oligos; gapped or mismatched anchors; hairpin self-priming. */
int64_t pcr_pool_conflicts_ext(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, int dimer_rule, float dimer_floor, const pcr_dimer_end3_args *ext,
	uint32_t *oligo_id, pcr_pool_conflict_ext *out, uint64_t cap);

/* ---- Probe hits: which products of a pool a panel's hydrolysis probes bind inside, and which sequences each assay detects */

/* One probe site inside one product (64 bytes). */
typedef struct {
	uint32_t plus_oligo, minus_oligo;   /* primer ids, pcr_pool_products' numbering */
	uint32_t probe;                     /* distinct-probe id (see probe_id) */
	uint32_t sequence;
	int32_t  begin, end, inner_start, inner_length;   /* the product, as pcr_product */
	int32_t  probe_loc5, probe_loc3;    /* the probe site, as pcr_site.loc5 / loc3: loc5 <= loc3 on either strand */
	uint32_t probe_strand;              /* 1 / 2 as pcr_site.strand */
	uint32_t intended;                  /* PCR_HIT_PRODUCT_INTENDED | PCR_HIT_PROBE_INTENDED */
	float    tm_plus, tm_minus, tm_probe;
	uint32_t flags;                     /* PCR_PRODUCT_PLUS_NO_TM | PCR_PRODUCT_MINUS_NO_TM | PCR_HIT_PROBE_NO_TM */
} pcr_probe_hit;

#define PCR_HIT_PRODUCT_INTENDED 1u     /* pcr_product.intended: {plus, minus} is a pool pair */
#define PCR_HIT_PROBE_INTENDED   2u     /* some pool pair i has {F_i, R_i} = {plus, minus} AND P_i = this probe */
#define PCR_HIT_PROBE_NO_TM      4u     /* the probe site is a PCR_SITE_NO_TM site: tm_probe = 0 */
#define PCR_NO_PROBE 0xFFFFFFFFu        /* probe_id of a pair without a probe */

/* Which products of a pool a probe binds inside, and which sequences each (F, R, probe) assay of the pool detects: the
 * products of pcr_pool_products_tm joined on the device with the probes' sites, floored, and reduced to one bitset per assay.
 *   Oligos.  oligo_id[2*n_pool] is exactly what pcr_pool_products writes for the same pool.  probes[i] is the probe of pair
 * i; an all-zero word means the pair has none, and probe_id[i] = PCR_NO_PROBE.  The other probe words get ids of their own,
 * 0 .. n_probe - 1, in order of first appearance: an id space separate from the primers'.  A probe word may equal a primer
 * word: it is then two oligos, each with its own concentration.  Distinct primers plus distinct probes must number at most
 * 2*PCR_POOL_MAX_PAIRS.  Probe oligos never take a primer role and primer oligos never take the probe role.
 *   Products.  pcr_pool_products_tm's products for the same handle state, pool, threshold, amplicon range, args,
 * template_strand and tm_floor: the eight product fields, tm_plus, tm_minus and the two product NO_TM flags of a record are
 * bit for bit those of that call's record.
 *   Probe sites.  The sites pcr_site_tm reports for the panel (P, P) of the distinct probes on the same DB at the same
 * threshold, with args->salt, primer_strand = probe_strand_conc and the same template_strand: tm_probe is that record's
 * tm_max, and PCR_SITE_NO_TM becomes PCR_HIT_PROBE_NO_TM with tm_probe = 0.  Sites on both strands count.  The DB must
 * hold them: fill it with pcr_select_sites over the pool plus one pair (P, P) per probe.
 *   A hit is a product and a site of any probe of the pool on the same sequence with p3 < probe_loc5 and probe_loc3 < m5,
 * where p3 = inner_start + 3 is the plus primer's 3' base and m5 = inner_start + inner_length - 8 the minus primer's 5' base
 * -- the strict non-overlap the two primers obey with each other -- that also passes probe_tm_floor <= 0 or
 * tm_probe >= probe_tm_floor (in float).
 *   Records are the hits, unique and sorted by (plus_oligo, minus_oligo, sequence, begin, end, probe, probe_loc5,
 * probe_strand).  Returns their number or a negative error; if it exceeds cap the contents of out are unspecified (cap = 0:
 * count only).  n_pool = 0 returns 0.
 *   detected may be NULL: n_pool x pcr_bitset_words(ctx, which) u64 in the bit layout of pcr_amplify, every row written in
 * full whenever the call returns >= 0, reduced on the device from the join and not from the records.  Row i of a pair with a
 * probe: bit s is set iff a hit on sequence s has {plus_oligo, minus_oligo} = {id(F_i), id(R_i)} in either orientation and
 * probe = probe_id[i].  Row i of a pair without a probe: bits_fr | bits_rf of row i of pcr_pool_products_tm at the same
 * tm_floor -- such a pair is detected by its product.  Pairs with equal (F, R) and different probes get different rows;
 * equal triples get equal rows.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in this order: unknown set or PCR_SET_MULTIPLEX; null
 * args, pool, probes, oligo_id or probe_id with n_pool > 0, or cap without out; n_pool > PCR_POOL_MAX_PAIRS; a negative
 * concentration (probe_strand_conc included); salt outside [1e-6, 1]; a primer that is empty, has a hole between its ends,
 * more than PCR_SITE_MAX_EXPANSIONS expansions or a zero strand concentration; the same for each probe (from
 * probe_strand_conc / degeneracy and template_strand); too many distinct oligos; a tm_floor that is not finite; a
 * probe_tm_floor that is not finite; then a null handle.  PCR_ERR_STATE without a word DB; PCR_ERR_CAPACITY for 2^31 or
 * more sites, (site, expansion) jobs, products or hits; PCR_ERR_RANGE if a trace-back fails inside the engine.  Changes
 * nothing other calls read.  On a handle with a target shard attached, sequence indices are local to the rank's block and no
 * collective is made (as pcr_pool_products). */
int64_t pcr_pool_probe_hits(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, const pcr_word128 *probes, uint32_t n_pool,
	float threshold, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float probe_strand_conc, float template_strand,
	float tm_floor, float probe_tm_floor, uint32_t *oligo_id, uint32_t *probe_id, pcr_probe_hit *out, uint64_t cap,
	uint64_t *detected);

/* pcr_pool_probe_hits inside the products that pass a 3'-end rule: the products are the ones pcr_pool_products_end3 keeps for
 * the same handle state, pool, threshold, amplicon range, args, template_strand, tm_floor and rule (its per-site quantities
 * and its test, after the floor).  The rule applies to the two primer sites of a product, never to the probe site: probe
 * sites, probe_tm_floor and the hit condition are pcr_pool_probe_hits'.  Hits exist only inside products that pass the rule,
 * and detected is reduced from those products: a row of a pair with a probe from their hits, a row of a pair without a probe
 * is bits_fr | bits_rf of pcr_pool_products_end3 at the same tm_floor and rule.
 *   Returns the number of hits or a negative error; cap, out and detected as pcr_pool_probe_hits.  rule = NULL or an
 * all-zero rule: out, detected and the return value are pcr_pool_probe_hits', byte for byte, and nothing is computed per
 * site.  args stays mandatory.
 *   PCR_ERR_ARG, from the arguments alone and before the handle: pcr_pool_probe_hits' checks in its order; then window,
 * min_clamp3 or max_end_mismatch above 32; use_taq_mama neither 0 nor 1; ident_threshold not finite or outside [0, 1]; then a
 * null handle.  PCR_ERR_STATE, PCR_ERR_CAPACITY and PCR_ERR_RANGE as pcr_pool_probe_hits.  Changes nothing other calls read.
 * On a handle with a target shard attached, sequence indices are local to the rank's block and no collective is made. */
int64_t pcr_pool_probe_hits_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, const pcr_word128 *probes, uint32_t n_pool,
	float threshold, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float probe_strand_conc, float template_strand,
	float tm_floor, float probe_tm_floor, const pcr_end3_rule *rule, uint32_t *oligo_id, uint32_t *probe_id, pcr_probe_hit *out,
	uint64_t cap, uint64_t *detected);

/* ---- Amplicons: the bases of products, their length and G+C, and which records spell one and the same amplicon */

/* What one product record spells (32 bytes). */
typedef struct {
	uint32_t length;        /* bases in the region */
	uint32_t gc;            /* bases whose code is C, G or S (2, 4, 6): only C and/or G possible */
	uint32_t other;         /* bases whose code is not A, C, G or T: ambiguity codes and EOS (0) */
	uint32_t flags;         /* PCR_AMPLICON_REVERSED */
	uint32_t amplicon;      /* class id, 0 .. n_classes-1, classes numbered by first appearance in input order */
	uint32_t first;         /* index of the first input record of this class */
	uint32_t copies;        /* input records in this class */
	uint32_t sequences;     /* distinct `sequence` values among them */
} pcr_amplicon_info;

#define PCR_AMPLICON_REVERSED 1u
#define PCR_REGION_PRODUCT 0   /* begin .. end: template bases under both primers included */
#define PCR_REGION_INSERT  1   /* strictly between the primers: inner_start+4 .. inner_start+inner_length-9 (p3+1 .. m5-1); may be empty */
#define PCR_REGION_INNER   2   /* inner_start .. inner_start+inner_length-1: the stretch PCR::extract_amplicon_seq cuts */

/* The bases of n product records, read on the device from the loaded set as it stands after every split (no word DB is
 * needed): per record its length, G+C and the class of records that spell the same bases; per class, on request, the bases.
 *   Input.  n contiguous pcr_product records, of which only sequence, begin, end, inner_start and inner_length are read: the
 * records of any of the product calls, of several calls, repeated, in any order, on active sequences or not.
 *   Region.  The region of record k is an interval of its sequence, chosen by `region` (PCR_REGION_*).  Every position must lie
 * in 0 .. length of the sequence - 1; only a PCR_REGION_INSERT may be empty (inner_length = 12: p3 + 1 = m5), wherever it is.
 *   Spelling.  The region's 4-bit codes, 5' -> 3' on the plus strand.  With canonical != 0 it is the smaller of that and its
 * reverse complement (A <-> T, C <-> G, hence R <-> Y, M <-> K, N -> N, EOS -> EOS), the two compared position by position with
 * the codes as unsigned integers; flags has PCR_AMPLICON_REVERSED iff the reverse complement is strictly smaller.  length, gc
 * and other do not depend on the strand.
 *   Classes.  Two records are in one class iff their spellings are equal: same length, same codes.  Oligo and sequence ids
 * play no part.  Classes are numbered by first appearance in input order.  The grouping is exact: records are grouped by a
 * hash on the device, every record is then compared base by base with the first of its group, and those that differ are
 * grouped by their bytes.  info[k] is written for every record; info may be NULL.
 *   Unique amplicons.  class_length[c] and class_byte_offset[c] are written for every class if their number is at most
 * class_cap.  packed4 (may be NULL) receives the spelling of each class -- that of its first record, canonical if asked -- two
 * codes per byte, high nibble first, an odd tail padded with 0, each class from a byte boundary in class order, if the bytes
 * needed are at most packed_cap: the triple pcr_load_sequences and pcr_multiplex_load take.  *packed_bytes (may be NULL)
 * always receives the bytes needed.  Nothing is written past n_classes entries or past the bytes needed; with class_cap
 * below n_classes, or packed_cap below the bytes needed, that output is left as it is.
 *   Returns n_classes, or a negative error; info is complete whenever it returns >= 0.  n = 0 returns 0.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in this order: unknown set or PCR_SET_MULTIPLEX; NULL
 * products with n > 0, class_cap > 0 with a NULL class array, or packed_cap > 0 with NULL packed4; unknown region; n >= 2^31;
 * then a null handle.  PCR_ERR_STATE if the set is not loaded.  With a handle, PCR_ERR_ARG naming the first record whose
 * sequence or region lies outside the set: checked on the host against the set's lengths before any launch.
 * PCR_ERR_CAPACITY if the packed output would reach 2^40 bytes.  Changes nothing other calls read.  On a handle with a target
 * shard attached, sequence indices are local to the rank's block and no collective is made (as pcr_pool_products). */
int64_t pcr_pool_amplicons(pcr_ctx *ctx, pcr_set which, const pcr_product *products, uint64_t n, int region, int canonical,
	pcr_amplicon_info *info,
	uint64_t *class_byte_offset, uint64_t *class_length, uint64_t class_cap,
	uint8_t *packed4, uint64_t packed_cap, uint64_t *packed_bytes);

/* ---- Probe candidates: the oligos that most sequences an assay amplifies hold between its primers */

/* One proposed probe of one assay (64 bytes). */
typedef struct {
	pcr_word128 word;            /* the probe, centred as assay oligos are stored: first base at slot (33 - length)/2 */
	uint32_t group;              /* the assay (caller's group id) */
	uint32_t length;             /* bases, len_min .. len_max */
	uint32_t gc;                 /* C + G bases */
	uint32_t sequences;          /* distinct `sequence` values among the group's records whose insert holds the word */
	uint32_t records;            /* distinct input records of the group whose insert holds it (twice in one insert: once) */
	uint32_t first_record;       /* the occurrence lowest in (sequence, record index, loc5, strand): its record index, */
	int32_t  first_loc5;         /*   the position in the sequence of the window's lowest base (loc3 = loc5 + length - 1), */
	uint32_t first_strand;       /*   1: the word is the plus strand's text there, 2: its reverse complement is */
	float tm, hairpin_tm, homodimer_tm, dG;   /* pcr_thermo's for this word; all 0 when args is NULL */
} pcr_probe_candidate;

#define PCR_PROBE_NO_5G   1u     /* the word's 5' base is not G */
#define PCR_PROBE_C_GE_G  2u     /* the word has at least as many C as G (picks the strand, with strands = 3) */
#define PCR_NO_GROUP 0xFFFFFFFFu /* group[] value of a record that takes no part */

/* Per assay, the oligos that occur in the inserts of the products it forms, pass the usual rules of a hydrolysis probe and
 * melt where a probe must: read on the device from the loaded set as it stands after every split (no word DB is needed).
 *   Input.  n contiguous pcr_product records, of which only sequence, inner_start and inner_length are read.  group[k] <
 * PCR_POOL_MAX_PAIRS is the assay of record k; PCR_NO_GROUP: the record takes no part and is not range-checked either; group =
 * NULL: every record is in group 0.  The region of a record is its PCR_REGION_INSERT (inner_start + 4, inner_length - 12
 * bases, may be empty), checked as that of the amplicon call above is.
 *   Occurrences.  For every participating record, every L in len_min .. len_max and every start with the window of L bases
 * inside the insert: a window all of whose codes are A, C, G or T is kept (one EOS or ambiguity code drops it).  A kept window
 * gives a strand-1 occurrence of the word spelled as read if strands & 1, and a strand-2 occurrence of its reverse complement if
 * strands & 2.
 *   Rules, on the word as oriented (a window may pass on one strand only).  An occurrence counts iff gc_min <= (float)gc /
 * (float)L <= gc_max compared in float, max_run == 0 or the longest run of one base is at most max_run, and the bits of `rules`
 * hold (PCR_PROBE_NO_5G, PCR_PROBE_C_GE_G).
 *   Candidates.  A candidate is a (group, word); occurrences on either strand, in any record of the group, belong to it.
 * `sequences` and `records` count distinct values, so a reverse-palindromic window -- two occurrences in one record -- counts
 * once.  A candidate is kept iff sequences >= min_sequences.
 *   Thermodynamics.  With args != NULL, tm, hairpin_tm, homodimer_tm and dG are bit for bit those pcr_thermo gives for the word
 * with the same check_homo_dimer and args (args->primer_strand is the probe's concentration), and the candidate is kept iff that
 * call's `valid` is 1.
 *   Records are the kept candidates sorted by group, and inside a group by (sequences descending, records descending, length
 * ascending, text ascending with A < C < G < T); per_group > 0 keeps the first per_group of each group after all filters.
 * Returns their number or a negative error; if it exceeds cap the contents of out are unspecified (cap = 0: count only).
 * n = 0 returns 0.
 *   PCR_ERR_ARG, from the arguments alone and before the handle, in this order: unknown set or PCR_SET_MULTIPLEX; NULL
 * products with n > 0, or cap without out; n >= 2^31; lengths outside 1 <= len_min <= len_max <= 32; strands not in 1 .. 3;
 * unknown bits in rules; gc_min or gc_max not finite, or gc_min > gc_max; with args: primer_strand <= 0, or salt outside
 * [1e-6, 1]; then a null handle.  With a handle: PCR_ERR_ARG for a group value that is neither below PCR_POOL_MAX_PAIRS nor
 * PCR_NO_GROUP; PCR_ERR_STATE if the set is not loaded (also with n = 0: the state is checked before the count, as in the
 * amplicon call above); PCR_ERR_ARG naming the first participating record whose sequence or
 * insert lies outside the set or whose insert is negative in length; PCR_ERR_CAPACITY if the windows to enumerate before the
 * rules -- the sum over the records and L of max(0, insert - L + 1), times the strands asked for -- number 2^28 or more, added
 * up on the host before anything is allocated; PCR_ERR_RANGE if a trace-back fails inside the engine.  Changes nothing other
 * calls read.  On a handle with a target shard attached, sequence indices are local to the rank's block and no collective is
 * made (as pcr_pool_products). */
int64_t pcr_pool_probe_candidates(pcr_ctx *ctx, pcr_set which, const pcr_product *products, const uint32_t *group, uint64_t n,
	uint32_t len_min, uint32_t len_max, uint32_t strands, uint32_t rules, uint32_t max_run, float gc_min, float gc_max,
	uint32_t min_sequences, const pcr_thermo_args *args, int check_homo_dimer, uint32_t per_group,
	pcr_probe_candidate *out, uint64_t cap);

/* ---- The multiplex compatibility filter of the trial loop (main.cpp:744-803), batched over the trial assays */

typedef struct {
	pcr_thermo_args thermo;        /* salt, primer_strand, max_dimer: PCR::multiplex_compatible (pcr_assay.cpp:815-852) */
	float background_threshold;    /* opt.background_threshold (find_multiplex_background_match) */
	int32_t use_taq_mama;
	float target_threshold;        /* opt.target_threshold, amplicon range: collect_unique_amplicons (main.cpp:787-789) */
	int32_t amp_min, amp_max;
} pcr_multiplex_screen_args;

/* For every trial assay t, what main.cpp:744-803 computes against the pool of accepted assays:
 *   compatible[t]      = every pool assay is multiplex_compatible with it (:748-752);
 *   multiplex_cover[t] = weighted_coverage of trial[t].find_multiplex_background_match over PCR_SET_MULTIPLEX (:767-771);
 *   pool_cover[t]      = weighted_coverage of the union, over the pool assays, of find_multiplex_background_match against the
 *                        trial's own unique amplicons (collect_unique_amplicons on the targets at target_threshold; amplicon
 *                        Sequences carry the default weight 1, so this is the number of unique amplicons some pool assay
 *                        matches; :786-803).
 * The two covers are computed for the trials with detail[t] != 0 (NULL: all) that are compatible; others get 0.  The reference
 * gates them on best_score < s and on max_background_cover as it walks the trials (:754, :778): the caller applies those to
 * the returned numbers.  One thermodynamics launch for all (trial, pool) pairs, one alignment pass for all trials over the
 * multiplex set, one for all pool assays over all trials' amplicons (loaded into an internal scratch set).  Needs the target
 * word DB selected for the trial batch (as pcr_collect_amplicons does). */
int pcr_multiplex_screen(pcr_ctx *ctx, const pcr_pair *trial, uint32_t n_trial, const pcr_pair *pool, uint32_t n_pool,
	const pcr_multiplex_screen_args *args, const uint8_t *detail, uint8_t *compatible, float *multiplex_cover, float *pool_cover);

/* ---- Random assay sampler (scope row f-2) */

/* The `Options` fields PCR::random_assay reads besides the thermodynamic ones (pcramp.h:21-30). */
typedef struct {
	int32_t primer_min, primer_max;  /* opt.primer_range */
	int32_t amp_min, amp_max;        /* opt.target_amplicon_range */
	double  max_degen;               /* opt.degen */
} pcr_sampler_args;

typedef struct {
	uint32_t sequence;               /* index of the sequence the assay was cut from */
	int32_t  f_start;                /* 0-based start of the forward primer */
	int32_t  amplicon_length;        /* the "Amplicon length" of the verbose line, pcr_assay.cpp:728 */
	uint32_t sequence_iterations;    /* "tried N seq ..." */
	uint32_t assay_iterations;       /* "... and M assays" (of the last sequence tried) */
} pcr_sample_info;

/* PCR::random_assay (pcr_assay.cpp:580-734) for n_trials fresh assays drawn one after the other from the
 * running glibc rand_r state *seed -- the body of the sampling loop main.cpp:544-550 as one thread executes
 * it (the caller obtains that thread's seed with pcr_host_rand_r(&global_seed), main.cpp:541-542).
 * Sequences, their active flags and their EOS splits are those of set `which` as loaded.  Validity
 * (is_valid with the homodimer test, max_dimer_tm) is evaluated on the device: the thermodynamic jobs of
 * every attempt that could start inside a window of the random stream go out as one launch.
 * pairs_out[i] = the centred assay of trial i; info_out is optional.  Where the reference throws
 * ("No active sequences found", "sequence length is too small!", "Unable to generate a valid initial
 * assay to test!", Sequence::subword out of bounds) an error code is returned with that text. */
int pcr_random_assays(pcr_ctx *ctx, pcr_set which, uint32_t *seed, uint32_t n_trials, const pcr_sampler_args *sampler,
	const pcr_thermo_args *thermo, pcr_pair *pairs_out, pcr_sample_info *info_out);

/* Word::max_overlap (word.h:38-91): the best ungapped diagonal of equal codes between two oligo words, as a
 * fraction of the longer one -- the oligo-reuse term of the multiplex Score (pcramp.h:158-208).  Host arithmetic. */
float pcr_host_max_overlap(const pcr_word128 *a, const pcr_word128 *b);

/* out[i] = max over both oligos of every pooled assay of Word::max_overlap(words[i], .) -- the inner loops of the
 * moves' oligo-reuse term (optimize_pcr.cpp:27-53, :129-139) for a batch of trial words; 0 for an empty pool. */
int pcr_host_pool_overlaps(const pcr_word128 *words, uint32_t n, const pcr_pair *pool, uint32_t n_pool, float *out);

/* PCR::compute_oligo_overlap (pcr_assay.cpp:736-754): both oligos of `assay` against both oligos of every pooled
 * assay, with MULTIPLEX_OLIGO_REUSE_BONUS (assay.h:19) for an identical oligo.  Host arithmetic. */
float pcr_host_oligo_overlap(const pcr_pair *assay, const pcr_pair *pool, uint32_t n_pool);

/* glibc rand_r (the reference's random source, sample.cpp:12), restated; usable without a GPU. */
uint32_t pcr_host_rand_r(uint32_t *seed);

/* ---- The local search behind the ABI, batched over trial assays (scope row f-1) */

/* The `Options` fields optimize() and its moves read (pcramp.h:83-128). */
typedef struct {
	double  max_degen;               /* opt.degen */
	int32_t primer_min, primer_max;  /* opt.primer_range */
	pcr_thermo_args thermo;          /* is_valid of the trial oligos: salt, primer_strand, tm range, max_hairpin (no dimer test there) */
	pcr_amplify_args target;         /* collect_threshold = target_threshold*target_search_multiplier, ident_threshold = target_threshold,
	                                    target amplicon range, use_taq_mama (optimize.cpp:61-77) */
	pcr_amplify_args background;     /* the same with the background thresholds and amplicon range */
	int32_t have_background;         /* 0: no background sequences, background coverage is 0 */
	int32_t use_multiplex;           /* opt.use_multiplex: multiplex background coverage (pcr_multiplex_load) and oligo reuse join the Score */
	float   multiplex_threshold;     /* opt.background_threshold, the threshold of the multiplex background coverage */
	int32_t n_moves;                 /* optimization_moves (main.cpp:82-95), at most 8, in order: PCR_MOVE_* */
	int32_t moves[8];
} pcr_optimize_args;

/* optimize() (optimize.cpp:14-207) for n assays at once -- the body of the parallel loop main.cpp:697-887 runs for every
 * trial assay of a design iteration.  The word DBs of the target set (and of the background set if have_background) must
 * have been built for these assays (pcr_select_words), as main.cpp builds them before it optimises.  All assays advance
 * in lockstep; per optimiser iteration ONE thermodynamics launch decides is_valid for every trial word of every assay
 * and ONE move-coverage pass per sequence set evaluates them (see pcr_optimize.inc).  pool = the assays designed so
 * far (use_multiplex).
 *   best_out[i]      : the best assay found for assays[i] (oligos centred as optimize.cpp:152 leaves them)
 *   score_out[3*i..] : its Score {target_coverage, background_coverage, oligo_overlap} (pcramp.h:158-208); optional
 *   iterations_out[i]: optimiser iterations it took; optional */
int pcr_optimize_batch(pcr_ctx *ctx, const pcr_pair *assays, uint32_t n, const pcr_optimize_args *args, const pcr_pair *pool, uint32_t n_pool,
	pcr_pair *best_out, float *score_out, uint32_t *iterations_out);

/* make_degenerate (optimize.cpp:356-398 -> PCR::maximize_degeneracy, pcr_assay.cpp:111-230) for n trial assays: the top-down start of
 * the local search (--optimize.top-down; main.cpp:709-721 calls it before optimize() and drops the trial when it returns false).
 * The target word DB must have been built for these assays (pcr_select_words).  Reads of args: max_degen (opt.degen), thermo (salt,
 * primer_strand, Tm range, max_hairpin, max_dimer: PCR::is_valid with the homodimer test, PCR::max_dimer_tm), target (collect
 * threshold, amplicon range, use_taq_mama).  assays[i] is replaced by the maximally degenerate assay; valid[i] = what the reference
 * returns (0: the greedy reduction ended non-degenerate with a heterodimer still above max_dimer).  Ties in the reference's
 * std::sort of the candidate amplicons by score are resolved by the same libstdc++ algorithm on the same initial order. */
int pcr_make_degenerate(pcr_ctx *ctx, pcr_pair *assays, uint32_t n, const pcr_optimize_args *args, uint8_t *valid);

/* optimization_move (optimize.cpp:303-352): ONE move (PCR_MOVE_*) of ONE oligo (side 0 = F, 1 = R) of one assay.
 * score_threshold (3 floats, optional): the Score trials are measured against; NULL = the unmodified assay's own Score,
 * as optimization_move computes it.  word_out = the winning trial word (not re-centred; all zero if no trial survives),
 * score_out = its Score (Score() = {-1e6, 1e6, 0} then), base_score_out (optional) = the unmodified assay's Score. */
int pcr_optimization_move(pcr_ctx *ctx, const pcr_pair *assay, int move, int side, const pcr_optimize_args *args, const pcr_pair *pool, uint32_t n_pool,
	const float *score_threshold, pcr_word128 *word_out, float *score_out, float *base_score_out);

/* ---- Assay-list writers (scope row f-4): the bytes `pcramp` writes to its output file.  Host only. */

/* What the writers read besides the assay itself (Options::output_format, opt.use_multiplex, the sequence records). */
typedef struct {
	int32_t json;                        /* 0 = Options::TEXT_OUTPUT, 1 = Options::JSON_OUTPUT (pcramp.h, --o.text / --o.json) */
	int32_t use_multiplex;               /* opt.use_multiplex (always true in v0.3, options.cpp:72): reused oligos are marked */
	uint32_t n_target, n_background;
	const char *const *target_deflines;       /* Sequence::defline(); keeps the leading '>' (parse_fasta.cpp:58) */
	const char *const *background_deflines;
	const uint64_t *target_lengths;           /* Sequence::length(), for sequence_summary (main.cpp:1326-1400) */
	const uint64_t *background_lengths;
} pcr_output;

/* One accepted assay as main.cpp:950-1113 writes it. */
typedef struct {
	uint32_t major_id, minor_id;              /* main.cpp:468-502 */
	pcr_pair assay;                           /* best_assay */
	float target_coverage, background_coverage;        /* best_score */
	float active_target_norm, active_background_norm;  /* summed weights of the active sequences (main.cpp:603,649) */
	uint32_t num_active_background;           /* main.cpp:565-569 */
	const uint64_t *target_match;             /* best_target_match: BitSet words, bit i%64 of word i/64 */
	const uint64_t *background_match;         /* best_background_match (may be NULL when there are no backgrounds) */
} pcr_assay_record;

/* All writers return the number of bytes of the text (the NUL is not counted) or a negative error; at most `cap`
 * bytes are stored (NUL-terminated when they fit), so a first call with cap = 0 sizes the buffer. */

/* PCR::write(ostream&) / write(ostream&, pool) / write_json(ostream&) / write_json(ostream&, pool), assay.h:288-375:
 * "F\tR\tD(F)=..;D(R)=.." with reused oligos in lower case (text), or the two primer objects with "recycled":True|False
 * (JSON).  use_multiplex = 0 selects the pool-less forms. */
int64_t pcr_format_oligos(const pcr_pair *assay, const pcr_pair *pool, uint32_t n_pool, int json, int use_multiplex,
	char *out, uint64_t cap);

/* Version, command line and seed (main.cpp:131-163), both sequence summaries (main.cpp:440-443) and, for JSON, the
 * opening of the assay array (main.cpp:460-462). */
int64_t pcr_format_header(const pcr_output *o, int argc, const char *const *argv, uint32_t seed, char *out, uint64_t cap);

/* The version, command line and seed lines of pcr_format_header alone (json = Options::JSON_OUTPUT): the reference writes and
 * flushes them before it reads its FASTA files (main.cpp:125-163), so they are all its output file holds when the ingest throws. */
int64_t pcr_format_preamble(int json, int argc, const char *const *argv, uint32_t seed, char *out, uint64_t cap);

/* What every design iteration writes BEFORE the search (main.cpp:504-519): the rule and "# Attempting to detect N
 * remaining targets" (text) or the record opening with its id (JSON).  The reference writes it even if the iteration
 * then finds no assay. */
int64_t pcr_format_iteration(const pcr_output *o, uint32_t assay_iteration, uint32_t major_id, uint32_t minor_id,
	uint32_t targets_remaining, char *out, uint64_t cap);

/* One accepted assay (main.cpp:950-1113): score line + "ASSAY.M.m" + oligos + "T-"/"B-" deflines (text), or the primer
 * objects + "target matches" + "background matches" (JSON).  pool = the assays accepted before this one. */
int64_t pcr_format_assay(const pcr_output *o, const pcr_assay_record *rec, const pcr_pair *pool, uint32_t n_pool,
	char *out, uint64_t cap);

/* The end of the file (main.cpp:1132-1264): targets still active (= not detected), background sequences any accepted
 * assay cross-reacted with (total_background = OR of the pool's background bitsets; may be NULL).  The JSON form
 * leaves the final "background matches" array unclosed when it is not empty, as the reference does (main.cpp:1235-1259). */
int64_t pcr_format_footer(const pcr_output *o, const uint8_t *target_active, const uint64_t *total_background,
	char *out, uint64_t cap);

/* ---- The design loop over all of the above (scope row f-7): what `pcramp` does between reading its FASTA files and closing
 * its output file (main.cpp:131-163, 440-443, 471-1264), one rank, one thread; over a target shard (pcr_shard_targets) the same
 * file, and with trial ranks attached (pcr_design_trial_ranks) the file of the reference's MPI mode at that world size. */

/* The `Options` fields that loop reads (pcramp.h:83-128; the pack filters are pcr_create's, sequences, weights and deflines
 * are the loaded sets' and pcr_output's). */
typedef struct {
	uint32_t num_assay;              /* --count: stop after this many design iterations */
	uint32_t num_trial;              /* --trial: trial assays per iteration (of this rank, main.cpp:66) */
	uint32_t seed;                   /* --seed: global_seed (main.cpp:113); one rand_r draw per iteration feeds the sampler */
	int32_t  top_down_search;        /* --optimize.top-down: make_degenerate before optimize() */
	int32_t  optimize_5, optimize_3; /* shifted candidates in select_words, the trim / grow moves */
	float    target_threshold, target_search_multiplier;
	float    background_threshold, background_search_multiplier;
	float    min_target_cover, max_background_cover;
	int32_t  target_amp_min, target_amp_max, background_amp_min, background_amp_max;
	int32_t  primer_min, primer_max; /* opt.primer_range; primer_min is also Options::min_oligo_length() */
	double   max_degen;              /* -d: > 1 enables the degeneracy moves (main.cpp:82-86) */
	pcr_thermo_args thermo;
	int32_t  use_taq_mama, use_multiplex;
} pcr_design_args;

/* Runs the design loop on the loaded PCR_SET_TARGET / PCR_SET_BACKGROUND sets (weights, active flags and EOS splits as they
 * stand; the call changes them exactly as the reference changes its target_seq: detected targets become inactive, accepted
 * amplicons split their targets) and leaves the bytes of the reference's output file in the handle (pcr_design_output).
 * argc / argv: the command line the header quotes.  pool_out (optional, pool_cap entries): the accepted assays in order;
 * n_pool_out: their number.  Where the reference throws (e.g. the sampler finds no valid assay) the error code and its text
 * are returned and the output so far stays readable. */
int pcr_design(pcr_ctx *ctx, const pcr_design_args *args, const pcr_output *o, int argc, const char *const *argv,
	pcr_pair *pool_out, uint32_t pool_cap, uint32_t *n_pool_out);
/* The text of the last pcr_design call (valid until the next one or pcr_destroy). */
const char *pcr_design_output(pcr_ctx *ctx, uint64_t *len_out);

/* ---- Host-only helpers (pure CPU arithmetic of the host half of the index build; usable
 * without a GPU; exercised by the `not gpu` tests). */

/* The irregular words of one sequence (Sequence::pack's partial / EOS-adjacent emissions,
 * sequence.cpp:155-179,198-263) whose size counter is >= min_oligo_length.  Returns the count. */
int64_t pcr_host_irregular_words(const uint8_t *packed4, uint64_t len, const pcr_params *params,
	uint32_t min_oligo_length, pcr_entry *out, uint64_t cap);

/* valid_out[p] (p < len) = 1 iff the 32-base window starting at p is a regular window that
 * Sequence::pack emits under `params` (all 32 bases non-EOS; GC and degeneracy filters pass). */
int pcr_host_window_valid(const uint8_t *packed4, uint64_t len, const pcr_params *params, uint8_t *valid_out);

/* select_words' candidate list (select_words.cpp:22-85): oligo words incl. 5'/3' slot shifts and
 * their floors unsigned(size*threshold).  Returns the count (may exceed cap). */
int64_t pcr_host_candidates(const pcr_pair *pairs, uint32_t n_pairs, int optimize_5, int optimize_3,
	float threshold, pcr_word128 *words_out, uint32_t *floors_out, uint64_t cap);

/* The seed scan's filter for one candidate orientation (host model of what pcr_select_words
 * uploads; no reference counterpart -- the reference counts every window, select_words.cpp:100-117).
 * `oligo` is matched as given against 32-base windows (slot k of the word <-> base k of the
 * window); a window reaches `floor` matching slots only if, for some returned seed i, its bases
 * off[i] .. off[i]+q[i]-1 spell codes[i] (2 bits per base, A,C,G,T = 0..3, first base in the low
 * bits).  Returns the seed count (may exceed cap), or -1 if the orientation cannot be seeded
 * (the bit-sliced scan handles it). */
int64_t pcr_host_orientation_seeds(const pcr_word128 *oligo, uint32_t floor, uint32_t *codes, uint8_t *q,
	uint8_t *off, uint64_t cap);

/* The seeds the position-index form of the scan reads for one orientation: the oligo's 10-gram seeds folded back into
 * 9-gram seeds with a constraint on the base behind the 9-gram (the index is sorted by it).  A window reaches `floor`
 * matching slots only if, for some returned seed i, its bases off[i] .. off[i]+8 spell codes[i] and the code of base
 * off[i]+9 lies in lo[i] .. hi[i] (A,C,G,T = 0..3; 0..3 = no constraint); every off[i] is at most 22.  Returns the seed
 * count (may exceed cap), or -1 if the oligo has no 10-gram block structure (the scan then reads its 9-gram seeds whole). */
int64_t pcr_host_orientation_fold_seeds(const pcr_word128 *oligo, uint32_t floor, uint32_t *codes, uint8_t *off,
	uint8_t *lo, uint8_t *hi, uint64_t cap);

/* The trial words of one local-search move of optimize_pcr.cpp for `oligo`, in the reference's order and
 * after its degeneracy / length gates (increase_degeneracy :17-19,:54-76; decrease_degeneracy :232-247;
 * trim5/trim3 :391-399; grow5/grow3 :671-673,:709-713), before is_valid (pcr_thermo) and the coverage
 * evaluation (pcr_move_coverage).  move: PCR_MOVE_*.  Host only.  Returns the count (may exceed cap). */
enum { PCR_MOVE_INCREASE_DEGENERACY = 0, PCR_MOVE_DECREASE_DEGENERACY = 1, PCR_MOVE_TRIM5 = 2, PCR_MOVE_TRIM3 = 3,
       PCR_MOVE_GROW5 = 4, PCR_MOVE_GROW3 = 5 };
int64_t pcr_host_move_trials(const pcr_word128 *oligo, int move, double max_degen, int primer_min, int primer_max,
	pcr_word128 *trials_out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PCRAMP_HIP_H */

// TEST INFRASTRUCTURE ONLY -- the parity checker.  Never linked into, imported by or shipped
// with the product (pcramp_amd/): only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may load liboracle.so.
//
// A plain scalar C++ restatement of the reference's primer x target evaluation path
// (LANL-Bioinformatics/PCRamp v0.3).  Each function cites the reference file:line it follows.
// Pinned against the real reference (oracle/_ref/libpcramp_ref.so, built from /root/reference
// by oracle/Makefile) and against the committed golden vectors in tests/golden/ -- see
// tests/test_oracle_vs_reference.py and tests/test_oracle_golden.py.
#ifndef PCR_ORACLE_H
#define PCR_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// Word layout == reference `Word` (word.cpp:11-16): slot k (0 = 5' end) is the nibble at bits
// (15 - k%16)*4 of w[k/16]; A=1 C=2 G=4 T=8, IUPAC = OR, EOS = 0 (base_table.h:11-28).
typedef struct { uint64_t w[2]; } orc_word;

typedef struct {
	uint64_t w[2];
	int32_t loc;      // WordMatch::loc (sequence.h:40)
	uint32_t index;   // sequence index
	uint32_t strand;  // 1 = plus, 2 = minus (sequence.h:27-32)
	uint32_t pad;
} orc_entry;

typedef struct {
	float target_threshold;     // opt.target_threshold            (pcramp.h:40)
	float search_multiplier;    // opt.target_search_multiplier    (pcramp.h:51)
	int32_t amp_min, amp_max;   // opt.target_amplicon_range       (pcramp.h:14-15)
	int32_t use_taq_mama;       // opt.use_taq_mama
	uint32_t pack_max_degen;    // opt.pack_max_degen              (pcramp.h:43)
	float pack_min_gc, pack_max_gc;
	int32_t min_primer;         // opt.primer_range.first -> min_oligo_length()
	int32_t optimize_5, optimize_3;
} orc_options;

// ---- Word primitives
unsigned orc_word_and(const uint64_t a[2], const uint64_t b[2]);           // word.cpp:68-154
unsigned orc_word_size(const uint64_t a[2]);                               // word.cpp:199-213
int orc_word_start(const uint64_t a[2]);                                   // word.h:256
int orc_word_stop(const uint64_t a[2]);                                    // word.h:273
double orc_word_degeneracy(const uint64_t a[2]);                           // word.h:97
int orc_word_from_string(const char *s, uint64_t out[2]);                  // word.h:234
void orc_word_center(uint64_t w[2]);                                       // word.h:392
void orc_word_complement(const uint64_t in[2], uint64_t out[2]);           // word.h:140
void orc_word_shift_left(uint64_t w[2]);                                   // word.cpp:215
void orc_word_shift_right(uint64_t w[2]);                                  // word.cpp:224
int orc_word_expand(const uint64_t in[2], uint64_t *out, int cap);         // word.h:525-647
float orc_taq_mama(unsigned p1, unsigned p2, unsigned t1, unsigned t2);    // word.cpp:249-294
float orc_word_max_overlap(const uint64_t a[2], const uint64_t b[2]);        // word.h:38-91
// PCR::compute_oligo_overlap (pcr_assay.cpp:736-754): assay = {F[2], R[2]}, pool = n x {F[2], R[2]}
float orc_oligo_overlap(const uint64_t assay[4], const uint64_t *pool, unsigned n_pool);

// ---- Sequence::pack (sequence.cpp:92-267).  '-' in `seq` = Base::EOS.
long orc_pack(const char *seq, unsigned index, unsigned degen_thr, float min_gc, float max_gc,
	unsigned min_len, orc_entry *out, long cap);

// ---- session (select_words + amplicon screen)
typedef struct orc_session orc_session;
orc_session *orc_session_create(void);
void orc_session_destroy(orc_session *s);
const char *orc_session_error(orc_session *s);
int orc_session_add_target(orc_session *s, const char *seq, float weight, int active);
int orc_session_add_target_packed(orc_session *s, const uint8_t *packed, uint64_t len, float weight, int active);
int orc_session_set_active(orc_session *s, unsigned idx, int active);
int orc_session_split(orc_session *s, unsigned idx, unsigned pos);         // sequence.h:228
void orc_session_set_options(orc_session *s, const orc_options *o);
// main.cpp:644-691 (pack + select_words per active sequence, then sort/keys)
long orc_session_select(orc_session *s, const uint64_t *pairs, unsigned n_pairs,
	float threshold, int min_len_override);
long orc_session_db_entries(orc_session *s, orc_entry *out, long cap);
// PCR::find_target_match (pcr_assay.cpp:544-578).  bits_out[i] in {0,1}.  If orient_out != NULL
// it receives, per target, bit0 = matched through {F(+),R(-)}, bit1 = through {R(+),F(-)}.
int orc_session_target_match(orc_session *s, const uint64_t pair[4], unsigned char *bits_out,
	unsigned char *orient_out);
// optimize.cpp:61-74: collect (search threshold) + update_identity + compute_coverage.
float orc_session_target_coverage(orc_session *s, const uint64_t pair[4]);
// main.cpp:1402-1418
// optimize_pcr.cpp move evaluation: coverage of each variant of one oligo (side 0 = F, 1 = R) over the
// BASE pair's candidate amplicons
int orc_session_move_coverage(orc_session *s, const uint64_t base[4], int side, const uint64_t *variants,
	unsigned n_variants, float *cov_out, unsigned char *orient_out);
// One complete local-search move as optimize() runs it for one oligo (optimize.cpp:61-140 +
// optimize_pcr.cpp): candidates of the base pair on the target session `t` and (optional) background
// session `b`, the move's trial words in the reference's order with its degeneracy / length gates,
// is_valid without the dimer check, target coverage, the coverage-bound shortcut, background coverage,
// Score comparison.  Non-multiplex.  move: 0 +degeneracy, 1 -degeneracy, 2 trim 5', 3 trim 3', 4 grow 5', 5 grow 3'.
typedef struct {
	int degen;                       // Options::degen (maximum oligo degeneracy)
	int primer_min, primer_max;      // Options::primer_range
	float salt, primer_strand, tm_min, tm_max, max_hairpin;
	float bg_threshold, bg_multiplier;
	int bg_amp_min, bg_amp_max;
} orc_move_options;
// out_score: target_coverage, background_coverage, oligo_overlap of the returned trial (the Score defaults
// -1e6, 1e6, 0 and an empty word if no trial survived); base_score_out (may be NULL): the base pair's.
int orc_optimization_move(orc_session *t, orc_session *b, const uint64_t pair[4], int move, int side,
	const orc_move_options *mo, uint64_t out_word[2], float out_score[3], float base_score_out[2]);

// optimize() (optimize.cpp:14-207), non-multiplex: the greedy local search around the moves; moves[] in the
// order of main.cpp:82-95.  pair_inout: the assay, replaced by the best one found.
int orc_optimize(orc_session *t, orc_session *b, uint64_t pair_inout[4], const int *moves, int n_moves,
	const orc_move_options *mo, float out_score[3], int *iterations_out);

// make_degenerate (optimize.cpp:356-398, PCR::maximize_degeneracy pcr_assay.cpp:111-230): pair_inout becomes the maximally
// degenerate assay; *valid_out = the reference's return value.  Reads degen, the thermodynamic limits (+ max_dimer).
int orc_make_degenerate(orc_session *t, uint64_t pair_inout[4], const orc_move_options *mo, float max_dimer, int *valid_out);

// PCR::collect_unique_amplicons (pcr_assay.cpp:756-813) over the session's word DB (orc_session_select first):
// bounds_out = n x {sequence, begin, end} in the reference's discovery order (AmpliconBounds, first/last base
// incl. primers); amp_codes_out = the unique amplicon stretches (non-primer part + padding, pcr_assay.cpp:489-497)
// as nibbles back to back, amp_len_out[k] their lengths, in the reference's sorted order.  Returns the number of
// bounds (may exceed cap_bounds), *n_amp_out = number of unique amplicons; <0 on error.
long orc_session_collect_amplicons(orc_session *s, const uint64_t pair[4], float threshold, int amp_min, int amp_max,
	unsigned *bounds_out, long cap_bounds, unsigned char *amp_codes_out, long cap_codes, unsigned *amp_len_out, long cap_amp,
	long *n_amp_out);
// Multiplex background coverage (pcr_assay.cpp:71-102, :304-336) with the session's sequences as the accepted
// amplicons: DB = pack of every sequence (session pack_max_degen, no G+C filter, min_primer; main.cpp:989-1001),
// candidates of `base`, then per trial word of the oligo on `side` update_identity + the distinct-key count.
int orc_multiplex_coverage(orc_session *s, const uint64_t base[4], int side, const uint64_t *variants, unsigned n_variants,
	float background_threshold, int use_taq_mama, float *cov_out, unsigned *n_keys_out);
int orc_optimization_move_multiplex(orc_session *t, orc_session *b, orc_session *amplicons, const uint64_t *pool, unsigned n_pool,
	const uint64_t pair[4], int move, int side, const orc_move_options *mo, uint64_t out_word[2], float out_score[3], float base_score_out[3]);
// optimize() with opt.use_multiplex (optimize.cpp:79-97, the multiplex blocks of every move in optimize_pcr.cpp)
int orc_optimize_multiplex(orc_session *t, orc_session *b, orc_session *amplicons, const uint64_t *pool, unsigned n_pool,
	uint64_t pair_inout[4], const int *moves, int n_moves, const orc_move_options *mo, float out_score[3]);
float orc_weighted_coverage(orc_session *s, const unsigned char *bits);

// ---- Smith-Waterman (SO::SeqOverlap, SmithWaterman + nucleic-acid mode; seq_overlap.cpp:347-609)
typedef struct {
	int16_t score;              // max_elem.M                      (seq_overlap.h:1321)
	int16_t q_start, q_stop;    // alignment_range_query           (seq_overlap.h:1289)
	int16_t t_start, t_stop;    // alignment_range_target          (seq_overlap.h:1301)
	uint8_t last1, last2;       // target_last_two_aligned         (seq_overlap.h:1266)
	uint8_t valid;              // 0: no cell reached the running maximum (the reference then leaves
	                            //    the coordinates stale; only `score` is defined)
	uint8_t pad;
} orc_sw_result;
// one lane: q/t are arrays of 4-bit codes
void orc_sw_align(const uint8_t *q, int qlen, const uint8_t *t, int tlen, orc_sw_result *out);
// pack_query_slots / pack_target_slots(Word) (seq_overlap.h:828,1099) then align
void orc_sw_align_words(const uint64_t q[2], const uint64_t t[2], orc_sw_result *out);
// PCR::find_background_match (background_match.cpp:7-166) over the session's sequences used as
// the background set (the DB must have been built with orc_session_select at
// background_threshold*multiplier and 0.9x min length, main.cpp:592-601).  Every candidate
// amplicon is evaluated.  The reference's loop tests `(i+1) >= num_seq` instead of the amplicon
// count (:122): it skips odd-indexed amplicons once their index reaches the number of sequences
// and, for an odd count below that, reads stale lanes and indexes past its deque.
// emulate_index_bug != 0 reproduces the skip (used only to pin this restatement against the
// compiled reference); the product implements emulate_index_bug == 0.  See DESIGN.md.
int orc_session_background_match(orc_session *s, const uint64_t pair[4], float bg_threshold, float bg_multiplier,
	int amp_min, int amp_max, int use_taq_mama, int emulate_index_bug, unsigned char *bits_out);
// The number of candidate amplicons PCR::collect_candidates (pcr_assay.cpp:12-69) forms for the pair at collect_threshold
// (= bg_threshold*bg_multiplier of the call above): the amplicon count that call loops over.  -1: error.
long orc_session_background_candidates(orc_session *s, const uint64_t pair[4], float collect_threshold, int amp_min, int amp_max);
// PCR::find_multiplex_background_match (background_match.cpp:168-295): the four oligo
// orientations against every sequence of the session (no DB needed).
int orc_session_multiplex_match(orc_session *s, const uint64_t pair[4], float bg_threshold, int use_taq_mama,
	unsigned char *bits_out);

// ---- nearest-neighbour thermodynamics (NucCruc, nuc_cruc.{h,cpp}) -- pcr_oracle_thermo.cpp
// out: [0] tm_pm_duplex, [1] dH, [2] dS, [3] dG(37C); [4] hairpin tm, [5] dH, [6] dS; [7] homodimer tm, [8] dH, [9] dS
int orc_thermo_full(const char *seq, float salt, float strand, float *out);
// out: tm, dH, dS of approximate_tm_heterodimer with strand(a, b) (nuc_cruc.h:818)
int orc_heterodimer_full(const char *a, const char *b, float salt, float strand_a, float strand_b, float *out);
// PCR::is_valid (valid_pcr.cpp:5-45): 1 pass, 0 fail
int orc_is_valid(const uint64_t word[2], float salt, float primer_strand, float tm_min, float tm_max,
	float max_hairpin, float max_dimer, int check_homo_dimer);
// PCR::max_dimer_tm (pcr_assay.cpp:232-269)
float orc_max_dimer_tm(const uint64_t pair[4], float salt, float primer_strand);
// PCR::multiplex_compatible (pcr_assay.cpp:815-852), a = this assay, b = argument
int orc_multiplex_compatible(const uint64_t a[4], const uint64_t b[4], float salt, float primer_strand, float max_dimer);

// ---- random assay sampler (scope row f-2)
typedef struct {
	int primer_min, primer_max;      // opt.primer_range
	int amp_min, amp_max;            // opt.target_amplicon_range
	double max_degen;                // opt.degen
	float salt, primer_strand, tm_min, tm_max, max_hairpin, max_dimer;
} orc_sampler_options;
// glibc rand_r (the reference's only random source, sample.cpp:12, pcr_assay.cpp:614-636; glibc 2.35
// stdlib/rand_r.c: three steps of the LCG x*1103515245+12345, 11+10+10 result bits).
unsigned orc_rand_r(unsigned *seed);
// PCR::random_assay (pcr_assay.cpp:580-734) n_trials times on one running seed, as the one-thread
// sampling loop of main.cpp:544-550 does.  pairs_out: n x {F[2], R[2]}, centred.  Returns 0, or <0
// where the reference throws (error text in orc_session_error).
int orc_random_assays(orc_session *s, unsigned *seed, unsigned n_trials, const orc_sampler_options *o, uint64_t *pairs_out);

#ifdef __cplusplus
}
#endif
#endif

// Amplicon screen kernels (included by pcr_device.hip): k_match, k_pair, k_pair_moves and the fused tail k_post.
// ============================================================================== amplicon screen
// match_words (optimize.cpp:291-301) of every assay oligo against every DB entry:
// mask[e][o/32] bit o%32 = entry matches oligo o at or above unsigned(size*thr^2).
// DB threads: thread g covers slot g%cap of the (g/cap)-th touched sequence.
__device__ __forceinline__ bool db_slot(uint32_t g, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, uint32_t &slot)
{
	if(g >= n) return false;
	const uint32_t seq = touched[g/cap];
	slot = seq*cap + g % cap;
	return slot < seg_hi[seq];
}

// One wave per touched sequence; a lane = (entry parity, oligo % 32): two DB entries against 32 oligos per
// step, the 64 compare results leave as one ballot.  (One lane per DB slot walked the oligo list serially:
// with a handful of filled slots per sequence that was a chain of dependent scalar loads, 20 us at C2.)
constexpr int MATCH_WAVES = 4;
__global__ __launch_bounds__(64*MATCH_WAVES) void k_match(const DevEntry *__restrict__ db, uint32_t n_touched, const uint32_t *__restrict__ n_touched_dev, uint32_t cap,
	const uint32_t *__restrict__ touched, const uint32_t *__restrict__ seg_hi, const OligoDev *__restrict__ oligos, uint32_t n_oligo,
	uint32_t mask_words, uint32_t *__restrict__ mask, uint32_t *__restrict__ status,
	const uint32_t *__restrict__ pub_counters, PassMail *pub_mail, uint32_t pub_seq)
{
	if(blockIdx.x == 0 && threadIdx.x == 0 && status) status[0] = 0;
	if(pub_mail && blockIdx.x == 0 && threadIdx.x < 64){        // the pass's counters -> host mailbox (k_publish's job in the fused pass)
		if(threadIdx.x < 4) pub_mail->counters[threadIdx.x] = pub_counters[threadIdx.x];
		__threadfence_system();
		__builtin_amdgcn_wave_barrier();
		if(threadIdx.x == 0) __hip_atomic_store((uint32_t *)&pub_mail->seq, pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	if(n_touched_dev) n_touched = *n_touched_dev;                // asynchronous passes: the host does not know it yet
	const uint32_t lane = threadIdx.x & 63u, sub = lane >> 5, ol = lane & 31u;
	for(uint32_t t_idx = blockIdx.x*MATCH_WAVES + (threadIdx.x >> 6);t_idx < n_touched;t_idx += gridDim.x*MATCH_WAVES){
	const uint32_t seq = touched[t_idx];
	const uint32_t lo = seq*cap, n_e = seg_hi[seq] - lo;         // filled slots [lo, seg_hi[seq])
	for(uint32_t e0 = 0;e0 < n_e;e0 += 2){
		const bool have = e0 + sub < n_e;
		const uint32_t i = lo + e0 + sub;
		Planes w; w.a = w.c = w.g = w.t = 0;
		if(have) w = db[i].w;
		for(uint32_t mw = 0;mw < mask_words;++mw){
			const uint32_t o = mw*32 + ol;
			bool ok = false;
			if(have && o < n_oligo){
				const Planes m = oligos[o].m;
				ok = (uint32_t)__popc((w.a & m.a) | (w.c & m.c) | (w.g & m.g) | (w.t & m.t)) >= oligos[o].floor2;
			}
			const uint64_t bal = __ballot(ok);
			if(have && ol == 0) mask[(size_t)i*mask_words + mw] = sub ? (uint32_t)(bal >> 32) : (uint32_t)bal;
		}
	}
	}
}

// k_match for a handful of oligos (the local search's base pair: 2): k_match's lane layout (2 entries x 32
// oligos per step) would leave 60 lanes idle and walk a 2 048-slot bucket in 1 024 steps; here a thread takes
// one DB slot and all (<= 32) oligos, one mask word per slot.
__global__ void k_match_few(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const OligoDev *__restrict__ oligos, uint32_t n_oligo, uint32_t *__restrict__ mask,
	uint32_t *__restrict__ status)
{
	__shared__ OligoDev sh[32];
	if(blockIdx.x == 0 && threadIdx.x == 0 && status) status[0] = 0;
	for(uint32_t i = threadIdx.x;i < n_oligo*(uint32_t)(sizeof(OligoDev)/4);i += blockDim.x) ((uint32_t *)sh)[i] = ((const uint32_t *)oligos)[i];
	__syncthreads();
	uint32_t e;
	if(!db_slot(blockIdx.x*blockDim.x + threadIdx.x, n, cap, touched, seg_hi, e)) return;
	const Planes w = db[e].w;
	uint32_t m = 0;
	for(uint32_t o = 0;o < n_oligo;++o){
		const Planes q = sh[o].m;
		if((uint32_t)__popc((w.a & q.a) | (w.c & q.c) | (w.g & q.g) | (w.t & q.t)) >= sh[o].floor2) m |= 1u << o;
	}
	mask[e] = m;
}

__device__ __forceinline__ uint32_t nibble_at(const Planes &p, int k)
{
	return ((p.a >> k) & 1u) | (((p.c >> k) & 1u) << 1) | (((p.g >> k) & 1u) << 2) | (((p.t >> k) & 1u) << 3);
}

__device__ __forceinline__ bool nondegen(uint32_t v) { return v == 1 || v == 2 || v == 4 || v == 8; }   // base_table.h:125

__device__ __forceinline__ int taq_idx(uint32_t v) { return (v == 2) ? 0 : (v == 4) ? 1 : (v == 1) ? 2 : 3; } // word.cpp:233

// update_identity for one (oligo, key) (optimize.cpp:209-261).  The pairing kernels test sqrtf(__fmul_rn(f, r)) >= thr:
// sqrtf is correctly rounded under the default flags, as the reference's sqrtf is; __fsqrt_rn is the bare v_sqrt_f32
// (about 1 ulp) here and refuses a pair whose exact score equals the threshold (an 18-mer with one mismatch at 17/18).
__device__ float identity(const OligoDev &o, const Planes &key, int use_taq)
{
	const uint32_t cnt = __popc((key.a & o.m.a) | (key.c & o.m.c) | (key.g & o.m.g) | (key.t & o.m.t));
	float id = __fmul_rn((float)cnt, o.norm);
	if(use_taq && nondegen(o.p1) && nondegen(o.p2)){
		const uint32_t t1 = nibble_at(key, o.stop - 1), t2 = nibble_at(key, o.stop);
		if(nondegen(t1) && nondegen(t2)){
			const float corr = fminf(1.0f, c_taq_mama[16*(4*taq_idx(t2) + taq_idx(t1)) + (4*taq_idx(o.p2) + taq_idx(o.p1))]);
			id = __fmul_rn(id, corr);
		}
	}
	return id;
}

// Sequence::has_split (sequence.cpp:304-330) on the plane store: any EOS in [start, start+n)?
__device__ bool has_split(const uint4 *__restrict__ planes, uint64_t base, int32_t start, int32_t n)
{
	int32_t pos = start;
	const int32_t end = start + n;
	while(pos < end){
		const uint32_t b = (uint32_t)pos >> 5, sh = (uint32_t)pos & 31;
		const uint4 v = planes[base + b];
		uint32_t nz = (v.x | v.y | v.z | v.w) >> sh;
		const int32_t span = min(32 - (int32_t)sh, end - pos);
		const uint32_t want = (span == 32) ? 0xFFFFFFFFu : ((1u << span) - 1u);
		if((nz & want) != want) return true;
		pos += span;
	}
	return false;
}

// One lane per plus-strand DB entry i; it walks the later entries j of the same sequence
// (sorted by WordMatch::loc, as assay.h:48-61) and, for every assay pair matched by both,
// applies find_amplicon_match (pcr_assay.cpp:338-441) and the identity test.
__global__ void k_pair(const DevEntry *__restrict__ db, uint32_t n, const uint32_t *__restrict__ n_touched_dev, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask, uint32_t mask_words, const OligoDev *__restrict__ oligos, uint32_t n_pairs,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, uint32_t *__restrict__ status)
{
	if(n_touched_dev) n = (*n_touched_dev)*cap;                                  // asynchronous passes
	for(uint32_t t = blockIdx.x*blockDim.x + threadIdx.x;t < n;t += gridDim.x*blockDim.x){
	uint32_t i;
	if(!db_slot(t, n, cap, touched, seg_hi, i)) continue;
	const DevEntry ei = db[i];
	if(ei.strand != 1) continue;
	if(!active[ei.seq]) continue;                                                // optimize.cpp:281
	const uint32_t hi = seg_hi[ei.seq];
	const int32_t L = (int32_t)len[ei.seq];
	const uint64_t base = blk_off[ei.seq];
	for(uint32_t j = i + 1;j < hi;++j){
		const DevEntry ej = db[j];
		if(ej.loc - ei.loc > amp_max + 128) break;   // beyond any admissible amplicon (slack: slots + end clamp)
		if(ej.strand != 2) continue;
		for(uint32_t w = 0;w < mask_words;++w){
			// oligo o = 2*pair + {0:F, 1:R}; F bits are the even bits, R bits the odd bits
			const uint32_t mi = mask[(size_t)i*mask_words + w], mj = mask[(size_t)j*mask_words + w];
			// orientation FR: F matches plus entry i, R matches minus entry j
			uint32_t fr = mi & (mj >> 1) & 0x55555555u;
			// orientation RF: R matches plus entry i, F matches minus entry j
			uint32_t rf = (mi >> 1) & mj & 0x55555555u;
			uint32_t any = fr | rf;
			while(any){
				const uint32_t bit = __ffs(any) - 1;
				any &= any - 1;
				const uint32_t pair = (w*32 + bit) >> 1;
				if(pair >= n_pairs) break;
				const OligoDev F = oligos[2*pair], R = oligos[2*pair + 1];
				for(int orient = 0;orient < 2;++orient){
					if(!(((orient == 0) ? fr : rf) >> bit & 1u)) continue;
					const OligoDev &P = (orient == 0) ? F : R;   // plus-role oligo
					const OligoDev &M = (orient == 0) ? R : F;   // minus-role oligo
					// pcr_assay.cpp:367-370 (WordMatch::template_loc3 / loc5, sequence.h:57-75)
					if(ei.loc + P.stop >= ej.loc - M.stop) continue;
					int32_t amp_start = ei.loc + P.start;
					const int32_t amp_stop = min(ej.loc - M.start, L - 1);
					int32_t amp_len = amp_stop - amp_start + 1;
					if(amp_len < amp_min || amp_len > amp_max) continue;
					if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
					if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }   // sequence.cpp:306 throw
					if(has_split(planes, base, amp_start, amp_len)) continue;
					const float f = identity(F, (orient == 0) ? ei.w : ej.w, use_taq);
					const float r = identity(R, (orient == 0) ? ej.w : ei.w, use_taq);
					if(sqrtf(__fmul_rn(f, r)) >= ident_thr){                // pcr_assay.cpp:572-576
						uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;
						atomicOr((unsigned long long *)&dst[(size_t)pair*bit_words + (ei.seq >> 6)], 1ull << (ei.seq & 63));
					}
				}
			}
		}
	}
	}
}

// Local-search move evaluation (optimize_pcr.cpp, e.g. :77-93): the candidate amplicons are those of the
// BASE pair (masks from k_match over {F, R}; geometry, has_split and the amplicon range from the base
// oligos, exactly k_pair's sweep); for each variant of the edited oligo (`side`) only that oligo's
// identity is re-evaluated (update_identity with the variant's own length and 3' bases), the other
// side keeps the base oligo's.  bits_*[v][seq].
//
// A thread owns one DB entry e matched by the EDITED base oligo and plays its role (plus strand: the
// plus-role primer, minus strand: the minus-role primer).  For a variant v the sequence is amplified through
// e iff some admissible partner p has sqrt(id(v, e) * id(other, p)) >= thr; rounding is monotone in each
// factor, so that is the test against the LARGEST partner identity: one sweep over the partners (geometry,
// has_split, the fixed oligo's identity), then one identity per variant -- partners + variants evaluations
// per entry instead of partners x variants.
__global__ void k_pair_moves(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask, const OligoDev *__restrict__ base /* F, R */,
	const OligoDev *__restrict__ variants, uint32_t n_variants, int side,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, uint32_t *__restrict__ status)
{
	const uint32_t t = blockIdx.x*blockDim.x + threadIdx.x;
	uint32_t e;
	if(!db_slot(t, n, cap, touched, seg_hi, e)) return;
	const uint32_t me = mask[e];                                                 // bit 0 = F, bit 1 = R (one mask word)
	if(!((me >> side) & 1u)) return;                                             // not a site of the edited oligo
	const DevEntry ee = db[e];
	if(!active[ee.seq]) return;                                                  // optimize.cpp:281
	const uint32_t lo = ee.seq*cap, hi = seg_hi[ee.seq];
	const int32_t L = (int32_t)len[ee.seq];
	const uint64_t blk_base = blk_off[ee.seq];
	const OligoDev F = base[0], R = base[1];
	const bool eos = has_eos[ee.seq] != 0;                                       // no EOS nibble in the sequence: has_split is false for every range
	const bool plus_role = (ee.strand == 1);
	// orientation 0 = {F plus, R minus}, 1 = {R plus, F minus}: the edited oligo sits on e's strand
	const int orient = plus_role ? side : 1 - side;
	const OligoDev &P = (orient == 0) ? F : R;                                   // plus-role oligo
	const OligoDev &M = (orient == 0) ? R : F;                                   // minus-role oligo
	const OligoDev &other = (side == 0) ? R : F;                                 // the oligo that is not edited
	const uint32_t other_bit = (side == 0) ? 1u : 0u;
	float best = -1.0f;
	// partners: minus-strand entries after e (e in the plus role) or plus-strand entries before it
	for(int64_t q = plus_role ? (int64_t)e + 1 : (int64_t)e - 1;plus_role ? (q < (int64_t)hi) : (q >= (int64_t)lo);q += plus_role ? 1 : -1){
		// only the partner's position is needed to leave the loop, only its mask to pass on: the 48-byte entry
		// (its word) is fetched for the few partners the fixed oligo matches
		const int32_t ploc = db[q].loc;
		const int32_t iloc = plus_role ? ee.loc : ploc;                           // plus-strand entry of the candidate amplicon
		const int32_t jloc = plus_role ? ploc : ee.loc;                           // minus-strand entry
		if(jloc - iloc > amp_max + 128) break;                                   // beyond any admissible amplicon (as k_pair)
		if(!((mask[q] >> other_bit) & 1u)) continue;
		if(db[q].strand != (plus_role ? 2u : 1u)) continue;
		if(iloc + P.stop >= jloc - M.stop) continue;                             // pcr_assay.cpp:367-370
		int32_t amp_start = iloc + P.start;
		const int32_t amp_stop = min(jloc - M.start, L - 1);
		int32_t amp_len = amp_stop - amp_start + 1;
		if(amp_len < amp_min || amp_len > amp_max) continue;
		if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
		if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }   // sequence.cpp:306 throw
		if(eos && has_split(planes, blk_base, amp_start, amp_len)) continue;
		best = fmaxf(best, identity(other, db[q].w, use_taq));
	}
	if(best < 0.0f) return;                                                      // no admissible amplicon through e
	uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;
	const uint64_t bit = 1ull << (ee.seq & 63);
	for(uint32_t v = 0;v < n_variants;++v){
		const float var = identity(variants[v], ee.w, use_taq);
		const float f = (side == 0) ? var : best, r = (side == 0) ? best : var;
		if(sqrtf(__fmul_rn(f, r)) >= ident_thr)                             // pcr_assay.cpp:285-287
			atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (ee.seq >> 6)], bit);
	}
}

// k_pair_moves for big buckets (backgrounds selected at a low threshold: hundreds to thousands of DB entries per
// sequence, of which a site's admissible partners are a small part): one workgroup per touched sequence.  It
// first compacts, in slot (= position) order, the entries the FIXED oligo matches into LDS records {position,
// identity with the fixed oligo (computed once per entry instead of once per site x partner), slot | strand};
// a site then finds its place in that list by bisection and sweeps records, not DB slots.  Same tests, same
// results as k_pair_moves (1.0 -> ms per launch at 2 000 x 10 kb, 2 048-slot buckets).
constexpr int PMS_THREADS = 256;
constexpr uint32_t PMS_MAX = 4096;               // slots per sequence this form takes (LDS: 48 KB of records)
struct PmsRec { int32_t loc; float id; uint32_t slot_strand; };

__global__ __launch_bounds__(PMS_THREADS) void k_pair_moves_seq(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint32_t *__restrict__ mask, const OligoDev *__restrict__ base /* F, R */,
	const OligoDev *__restrict__ variants, uint32_t n_variants, int side,
	const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off, const uint64_t *__restrict__ len,
	const uint8_t *__restrict__ active, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, uint32_t *__restrict__ status)
{
	__shared__ PmsRec rec[PMS_MAX];
	__shared__ uint32_t wave_count[PMS_THREADS/64];
	const uint32_t seq = touched[blockIdx.x];
	if(!active[seq]) return;                                                     // optimize.cpp:281 (uniform for the workgroup)
	const uint32_t lo = seq*cap, n_e = seg_hi[seq] - lo;
	const OligoDev F = base[0], R = base[1];
	const OligoDev &other = (side == 0) ? R : F;                                 // the oligo that is not edited
	const uint32_t other_bit = (side == 0) ? 1u : 0u;
	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
	uint32_t n_rec = 0;
	for(uint32_t c0 = 0;c0 < n_e;c0 += PMS_THREADS){                             // ordered compaction of the fixed oligo's sites
		const uint32_t slot = c0 + tid;
		const bool is = (slot < n_e) && ((mask[lo + slot] >> other_bit) & 1u);
		const unsigned long long b = __ballot(is);
		if(lane == 0) wave_count[wave] = (uint32_t)__popcll(b);
		__syncthreads();
		uint32_t before = 0, total = 0;
		for(uint32_t w = 0;w < PMS_THREADS/64;++w){ if(w < wave) before += wave_count[w]; total += wave_count[w]; }
		if(is){
			const DevEntry e = db[lo + slot];
			PmsRec r; r.loc = e.loc; r.id = identity(other, e.w, use_taq); r.slot_strand = slot | (e.strand << 16);
			rec[n_rec + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = r;
		}
		n_rec += total;
		__syncthreads();
	}
	if(n_rec == 0) return;
	const int32_t L = (int32_t)len[seq];
	const uint64_t blk_base = blk_off[seq];
	const bool eos = has_eos[seq] != 0;
	for(uint32_t c0 = 0;c0 < n_e;c0 += PMS_THREADS){
		const uint32_t slot = c0 + tid;
		if(slot >= n_e || !((mask[lo + slot] >> side) & 1u)) continue;           // not a site of the edited oligo
		const DevEntry ee = db[lo + slot];
		const bool plus_role = (ee.strand == 1);
		const int orient = plus_role ? side : 1 - side;                          // 0 = {F plus, R minus}, 1 = {R plus, F minus}
		const OligoDev &P = (orient == 0) ? F : R;
		const OligoDev &M = (orient == 0) ? R : F;
		// first record after this slot (plus role) / last record before it (minus role)
		uint32_t a = 0, z = n_rec;
		while(a < z){ const uint32_t m = (a + z) >> 1; if((rec[m].slot_strand & 0xFFFFu) < slot + (plus_role ? 1u : 0u)) a = m + 1; else z = m; }
		// plus role: a = first index with rec.slot > slot; minus role: a = first index with rec.slot >= slot, so a - 1 is the last before
		float best = -1.0f;
		for(int64_t k = plus_role ? (int64_t)a : (int64_t)a - 1;plus_role ? (k < (int64_t)n_rec) : (k >= 0);k += plus_role ? 1 : -1){
			const PmsRec r = rec[k];
			const int32_t iloc = plus_role ? ee.loc : r.loc;
			const int32_t jloc = plus_role ? r.loc : ee.loc;
			if(jloc - iloc > amp_max + 128) break;                               // beyond any admissible amplicon (as k_pair)
			if((r.slot_strand >> 16) != (plus_role ? 2u : 1u)) continue;
			if(iloc + P.stop >= jloc - M.stop) continue;                         // pcr_assay.cpp:367-370
			int32_t amp_start = iloc + P.start;
			const int32_t amp_stop = min(jloc - M.start, L - 1);
			int32_t amp_len = amp_stop - amp_start + 1;
			if(amp_len < amp_min || amp_len > amp_max) continue;
			if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
			if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(status, 1u); continue; }   // sequence.cpp:306 throw
			if(eos && has_split(planes, blk_base, amp_start, amp_len)) continue;
			best = fmaxf(best, r.id);
		}
		if(best < 0.0f) continue;
		uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;
		const uint64_t bit = 1ull << (seq & 63);
		for(uint32_t v = 0;v < n_variants;++v){
			const float var = identity(variants[v], ee.w, use_taq);
			const float f = (side == 0) ? var : best, r2 = (side == 0) ? best : var;
			if(sqrtf(__fmul_rn(f, r2)) >= ident_thr)                        // pcr_assay.cpp:285-287
				atomicOr((unsigned long long *)&dst[(size_t)v*bit_words + (seq >> 6)], bit);
		}
	}
}

// The whole tail of a fused pass in ONE launch (k_touched + k_finalize + k_match + k_pair, for the common
// case of 64-slot buckets and <= 128 oligos): one wave per SEQUENCE of the set -- a wave whose sequence
// collected no hit leaves at once -- keeps the final-maximum hits, sorts and dedupes them (one key per lane),
// materialises the sequence's DB entries (global, for later callers, and LDS), builds their oligo masks and
// runs k_pair's sweep over them out of LDS.  The touched list is not built (ensure_touched() does it on
// demand); block 0 publishes the pass's counters (overflow flag, fill) at kernel start, when every scan is
// complete.  The has_split range error (sequence.cpp:306, unreachable with clamped amplicon ends) is noted in
// counters[1] but, as with pcr_amplify_device, the asynchronous entry points do not report it.
// waves per workgroup: a template parameter (r02: 16 waves 70.3 vs 68.2 us per pass at C2; 4 the same as 8; r03: 4, 8 and 16
// within the noise, profiles/dbg/r03_ab_post_waves.txt): the pass launches 8
constexpr uint32_t POST_CAP = 64, POST_MASK_WORDS = 4;
// (what the match and pair steps read of an entry: half a DevEntry -- 30 KB of LDS per workgroup instead of 42, four workgroups =
// all 32 waves of a CU resident instead of three)
struct PostEnt { Planes w; int32_t loc; uint32_t strand; };
template<int POST_WAVES>
struct PostShared {
	OligoDev ol[32*POST_MASK_WORDS];           // the pass's oligo table, staged once per workgroup
	uint64_t keys[POST_WAVES][POST_CAP]; PostEnt ent[POST_WAVES][POST_CAP]; uint32_t msk[POST_WAVES][POST_CAP][POST_MASK_WORDS];
};

// (the tail of one pass as the workgroups of one launch row run it: k_post is this and nothing else, k_post_pair runs it once per row)
template<int POST_WAVES>
__device__ __forceinline__ void post_pass(PostShared<POST_WAVES> &sh, const Hit *__restrict__ hits, uint32_t *__restrict__ seq_count,
	const uint32_t *__restrict__ best, uint32_t ncand, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off, DevEntry *__restrict__ db, uint32_t *__restrict__ seg_hi,
	uint32_t *__restrict__ counters, uint32_t epoch, uint32_t n_seq,
	const OligoDev *__restrict__ oligos, uint32_t n_pairs, uint32_t mask_words,
	const uint64_t *__restrict__ len, const uint8_t *__restrict__ active, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, PassMail *pub_mail, uint32_t pub_seq)
{
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	if(pub_mail && blockIdx.x == 0 && wave == 0){              // every scan of the pass is complete: its counters -> host mailbox
		if(lane < 4) pub_mail->counters[lane] = (lane == 3) ? N_TOUCHED_UNKNOWN_DEV : counters[lane];
		__threadfence_system();
		__builtin_amdgcn_wave_barrier();
		if(lane == 0) __hip_atomic_store((uint32_t *)&pub_mail->seq, pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	// This kernel leaves the pass's control block the way the next pass needs it -- counters zero (once published), every fill
	// zero, the segment end of a sequence without hits zero -- so that a fused pass that follows needs no clearing launch.
	if(blockIdx.x == 0 && wave == 0 && lane < 4) counters[lane] = 0;
	const uint32_t seq = blockIdx.x*POST_WAVES + wave;
	const uint32_t n_raw = (seq < n_seq) ? seq_count[seq] : 0u;
	const uint32_t n = min(n_raw, POST_CAP);
	if(seq < n_seq && lane == 0){
		if(n_raw) seq_count[seq] = 0;
		else seg_hi[seq] = 0;
	}
	// what the later stages need of the sequence is requested now, beside its fill, not in front of each stage (the wave's life
	// is a chain of dependent loads)
	const uint32_t seq_c = min(seq, n_seq - 1u);
	const uint64_t base = blk_off[seq_c];
	const int32_t L = (int32_t)len[seq_c];
	const uint32_t is_active = active[seq_c];
	// a workgroup with at least one busy wave stages the oligo table (a chain of dependent scalar loads per
	// oligo made the match loop the longest part of the wave's life)
	if(__syncthreads_or((int)n)){
		const uint32_t nw = 2*n_pairs*(uint32_t)(sizeof(OligoDev)/4);
		for(uint32_t i = threadIdx.x;i < nw;i += 64*POST_WAVES) ((uint32_t *)sh.ol)[i] = ((const uint32_t *)oligos)[i];
		__syncthreads();
	}
	if(n == 0) return;                                          // seg_hi[seq] stays 0 = empty
	uint64_t *keys = sh.keys[wave];
	PostEnt *ent = sh.ent[wave];
	// ---- k_finalize: one key per lane
	uint64_t k = ~0ull;
	if(lane < n){
		const Hit h = hits[(size_t)seq*POST_CAP + lane];
		if(((epoch << 8) | h.cnt) == best[(size_t)seq*ncand + h.cand]) k = h.key;
	}
	keys[lane] = k;
	wave_sync();
	uint32_t np2 = 1; while(np2 < n) np2 <<= 1;                // sentinels beyond n are already in place: sort only the first np2 keys
	for(uint32_t kk = 2;kk <= np2;kk <<= 1){
		for(uint32_t j = kk >> 1;j > 0;j >>= 1){
			const uint32_t l = lane ^ j;
			if(l > lane && l < np2){
				const uint64_t a = keys[lane], b = keys[l];
				const bool up = ((lane & kk) == 0);
				if((a > b) == up){ keys[lane] = b; keys[l] = a; }
			}
			wave_sync();
		}
	}
	k = keys[lane];
	const bool distinct = k != ~0ull && (lane == 0 || keys[lane - 1] != k);
	const uint64_t dmask = __ballot(distinct);
	const uint32_t run = (uint32_t)__builtin_popcountll(dmask);
	const uint32_t rank = (uint32_t)__builtin_popcountll(dmask & ((1ull << lane) - 1ull));
	if(lane == 0) seg_hi[seq] = seq*POST_CAP + run;
	if(distinct){
		DevEntry e;
		materialise_entry_at(k, planes, base, irr, irr_off, e);
		db[(size_t)seq*POST_CAP + rank] = e;
		PostEnt pe; pe.w = e.w; pe.loc = e.loc; pe.strand = e.strand;
		ent[rank] = pe;
	}
	wave_sync();
	if(n_pairs == 0) return;
	// ---- k_match: lane = oligo (64 at a time, its masks in registers), the sequence's few entries walked one after the other
	// with their word broadcast out of LDS, 64 compares per ballot.  (Lane = entry with the oligos as scalar operands kept
	// ~15 % of the lanes busy: a sequence has ~10 entries, a pass 100 oligos.)
	const uint32_t n_oligo = 2*n_pairs;
	PostEnt me; me.w.a = me.w.c = me.w.g = me.w.t = 0; me.loc = 0; me.strand = 0;
	if(lane < run) me = ent[lane];
	for(uint32_t g = 0;2*g < mask_words;++g){
		const uint32_t o = g*64 + lane;
		Planes m; m.a = m.c = m.g = m.t = 0; uint32_t fl = 0xFFFFFFFFu;                 // (no oligo: never matches)
		if(o < n_oligo){ m = sh.ol[o].m; fl = sh.ol[o].floor2; }
		for(uint32_t e = 0;e < run;++e){
			const Planes w = ent[e].w;                                                   // the same address for all lanes: one LDS broadcast
			const uint32_t cnt = __popc((w.a & m.a) | (w.c & m.c) | (w.g & m.g) | (w.t & m.t));
			const uint64_t bal = __ballot(cnt >= fl);
			if(lane == 0){
				sh.msk[wave][e][2*g] = (uint32_t)bal;
				if(2*g + 1 < mask_words) sh.msk[wave][e][2*g + 1] = (uint32_t)(bal >> 32);
			}
		}
	}
	wave_sync();
	// ---- k_pair: lane = plus-strand entry i, walks the later entries of the sequence
	if(lane >= run || me.strand != 1 || !is_active) return;             // optimize.cpp:281
	for(uint32_t j = lane + 1;j < run;++j){
		const PostEnt ej = ent[j];
		if(ej.loc - me.loc > amp_max + 128) break;
		if(ej.strand != 2) continue;
		for(uint32_t w = 0;w < mask_words;++w){
			const uint32_t mi = sh.msk[wave][lane][w], mj = sh.msk[wave][j][w];
			uint32_t fr = mi & (mj >> 1) & 0x55555555u;
			uint32_t rf = (mi >> 1) & mj & 0x55555555u;
			uint32_t any = fr | rf;
			while(any){
				const uint32_t bit = __ffs(any) - 1;
				any &= any - 1;
				const uint32_t pair = (w*32 + bit) >> 1;
				if(pair >= n_pairs) break;
				const OligoDev F = sh.ol[2*pair], R = sh.ol[2*pair + 1];
				for(int orient = 0;orient < 2;++orient){
					if(!(((orient == 0) ? fr : rf) >> bit & 1u)) continue;
					const OligoDev &P = (orient == 0) ? F : R;   // plus-role oligo
					const OligoDev &M = (orient == 0) ? R : F;   // minus-role oligo
					if(me.loc + P.stop >= ej.loc - M.stop) continue;                       // pcr_assay.cpp:367-370
					int32_t amp_start = me.loc + P.start;
					const int32_t amp_stop = min(ej.loc - M.start, L - 1);
					int32_t amp_len = amp_stop - amp_start + 1;
					if(amp_len < amp_min || amp_len > amp_max) continue;
					if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
					if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(&counters[1], 1u); continue; }   // sequence.cpp:306 throw
					if(has_split(planes, base, amp_start, amp_len)) continue;
					const float f = identity(F, (orient == 0) ? me.w : ej.w, use_taq);
					const float r = identity(R, (orient == 0) ? ej.w : me.w, use_taq);
					if(sqrtf(__fmul_rn(f, r)) >= ident_thr){                        // pcr_assay.cpp:572-576
						uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;
						atomicOr((unsigned long long *)&dst[(size_t)pair*bit_words + (seq >> 6)], 1ull << (seq & 63));
					}
				}
			}
		}
	}
}

template<int POST_WAVES>
__global__ __launch_bounds__(64*POST_WAVES) void k_post(const Hit *__restrict__ hits, uint32_t *__restrict__ seq_count,
	const uint32_t *__restrict__ best, uint32_t ncand, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off, DevEntry *__restrict__ db, uint32_t *__restrict__ seg_hi,
	uint32_t *__restrict__ counters, uint32_t epoch, uint32_t n_seq,
	const OligoDev *__restrict__ oligos, uint32_t n_pairs, uint32_t mask_words,
	const uint64_t *__restrict__ len, const uint8_t *__restrict__ active, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, PassMail *pub_mail, uint32_t pub_seq)
{
	__shared__ PostShared<POST_WAVES> sh;
	post_pass<POST_WAVES>(sh, hits, seq_count, best, ncand, planes, blk_off, irr, irr_off, db, seg_hi, counters, epoch, n_seq, oligos, n_pairs, mask_words,
		len, active, amp_min, amp_max, ident_thr, use_taq, bits_fr, bits_rf, bit_words, pub_mail, pub_seq);
}

// The tails of two passes of different handles in one launch: row blockIdx.y runs its pass's tail, gridDim.x is the larger of the two
// workgroup counts and a workgroup beyond its own pass's count leaves at once.  Each row publishes its own mailbox and leaves its
// own control block clean; the rows share nothing.
struct PostRow {
	const Hit *hits; uint32_t *seq_count; const uint32_t *best; uint32_t ncand; const uint4 *planes; const uint64_t *blk_off;
	const IrrDev *irr; const uint32_t *irr_off; DevEntry *db; uint32_t *seg_hi; uint32_t *counters; uint32_t epoch, n_seq;
	const OligoDev *oligos; uint32_t n_pairs, mask_words; const uint64_t *len; const uint8_t *active; int32_t amp_min, amp_max; float ident_thr; int use_taq;
	uint64_t *bits_fr, *bits_rf; uint64_t bit_words; PassMail *pub_mail; uint32_t pub_seq;
};
template<int POST_WAVES>
__device__ __forceinline__ void post_row(PostShared<POST_WAVES> &sh, const PostRow &R)
{
	if(blockIdx.x*POST_WAVES >= R.n_seq) return;               // (uniform per workgroup, before any barrier)
	post_pass<POST_WAVES>(sh, R.hits, R.seq_count, R.best, R.ncand, R.planes, R.blk_off, R.irr, R.irr_off, R.db, R.seg_hi, R.counters, R.epoch, R.n_seq,
		R.oligos, R.n_pairs, R.mask_words, R.len, R.active, R.amp_min, R.amp_max, R.ident_thr, R.use_taq, R.bits_fr, R.bits_rf, R.bit_words, R.pub_mail, R.pub_seq);
}
template<int POST_WAVES>
__global__ __launch_bounds__(64*POST_WAVES) void k_post_pair(PostRow A, PostRow B)
{
	__shared__ PostShared<POST_WAVES> sh;
	if(blockIdx.y == 0) post_row<POST_WAVES>(sh, A);            // (uniform per workgroup)
	else post_row<POST_WAVES>(sh, B);
}

// The same tail for buckets that have grown to 128 or 256 slots (5'/3' shift candidates multiply the words
// per site): every lane owns CAP/64 keys, the sort / rank / match / pair steps loop over them.
template<uint32_t CAP, int WAVES>
struct PostSharedBig {
	OligoDev ol[32*POST_MASK_WORDS];
	uint64_t keys[WAVES][CAP]; DevEntry ent[WAVES][CAP]; uint32_t msk[WAVES][CAP][POST_MASK_WORDS]; uint32_t part[WAVES][64];
};

template<uint32_t CAP, int WAVES>
__global__ __launch_bounds__(64*WAVES) void k_post_big(const Hit *__restrict__ hits, const uint32_t *__restrict__ seq_count,
	const uint32_t *__restrict__ best, uint32_t ncand, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const IrrDev *__restrict__ irr, const uint32_t *__restrict__ irr_off, DevEntry *__restrict__ db, uint32_t *__restrict__ seg_hi,
	uint32_t *__restrict__ counters, uint32_t epoch, uint32_t n_seq,
	const OligoDev *__restrict__ oligos, uint32_t n_pairs, uint32_t mask_words,
	const uint64_t *__restrict__ len, const uint8_t *__restrict__ active, int32_t amp_min, int32_t amp_max, float ident_thr, int use_taq,
	uint64_t *__restrict__ bits_fr, uint64_t *__restrict__ bits_rf, uint64_t bit_words, PassMail *pub_mail, uint32_t pub_seq)
{
	__shared__ PostSharedBig<CAP, WAVES> sh;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	if(pub_mail && blockIdx.x == 0 && wave == 0){
		if(lane < 4) pub_mail->counters[lane] = (lane == 3) ? N_TOUCHED_UNKNOWN_DEV : counters[lane];
		__threadfence_system();
		__builtin_amdgcn_wave_barrier();
		if(lane == 0) __hip_atomic_store((uint32_t *)&pub_mail->seq, pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
	const uint32_t seq = blockIdx.x*WAVES + wave;
	const uint32_t n = (seq < n_seq) ? min(seq_count[seq], CAP) : 0u;
	if(__syncthreads_or((int)n)){
		const uint32_t nw = 2*n_pairs*(uint32_t)(sizeof(OligoDev)/4);
		for(uint32_t i = threadIdx.x;i < nw;i += 64*WAVES) ((uint32_t *)sh.ol)[i] = ((const uint32_t *)oligos)[i];
		__syncthreads();
	}
	if(n == 0) return;
	uint64_t *keys = sh.keys[wave];
	DevEntry *ent = sh.ent[wave];
	uint32_t *part = sh.part[wave];
	uint32_t np2 = 1; while(np2 < n) np2 <<= 1;
	for(uint32_t i = lane;i < np2;i += 64){
		uint64_t k = ~0ull;
		if(i < n){
			const Hit h = hits[(size_t)seq*CAP + i];
			if(((epoch << 8) | h.cnt) == best[(size_t)seq*ncand + h.cand]) k = h.key;
		}
		keys[i] = k;
	}
	wave_sync();
	for(uint32_t kk = 2;kk <= np2;kk <<= 1){
		for(uint32_t j = kk >> 1;j > 0;j >>= 1){
			for(uint32_t i = lane;i < np2;i += 64){
				const uint32_t l = i ^ j;
				if(l > i){
					const uint64_t a = keys[i], b = keys[l];
					const bool up = ((i & kk) == 0);
					if((a > b) == up){ keys[i] = b; keys[l] = a; }
				}
			}
			wave_sync();
		}
	}
	// distinct, non-sentinel keys -> ranks (each lane owns a contiguous chunk)
	const uint32_t chunk = (np2 + 63)/64;
	const uint32_t lo = min(np2, lane*chunk), hi = min(np2, lo + chunk);
	uint32_t cnt = 0;
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = keys[i];
		if(k != ~0ull && (i == 0 || keys[i - 1] != k)) ++cnt;
	}
	part[lane] = cnt;
	wave_sync();
	uint32_t rank = 0, run = 0;
	for(uint32_t t = 0;t < 64;++t){ const uint32_t c = part[t]; if(t < lane) rank += c; run += c; }
	if(lane == 0) seg_hi[seq] = seq*CAP + run;
	for(uint32_t i = lo;i < hi;++i){
		const uint64_t k = keys[i];
		if(k != ~0ull && (i == 0 || keys[i - 1] != k)){
			DevEntry e;
			materialise_entry(k, planes, blk_off, irr, irr_off, e);
			db[(size_t)seq*CAP + rank] = e;
			ent[rank] = e;
			++rank;
		}
	}
	wave_sync();
	if(n_pairs == 0) return;
	const uint32_t n_oligo = 2*n_pairs;
	for(uint32_t e = lane;e < run;e += 64){                       // k_match
		const DevEntry me = ent[e];
		for(uint32_t mw = 0;mw < mask_words;++mw){
			uint32_t bits = 0;
			const uint32_t o_end = min(n_oligo, (mw + 1)*32);
#pragma unroll 4
			for(uint32_t o = mw*32;o < o_end;++o){
				const Planes m = sh.ol[o].m;
				const uint32_t c = __popc((me.w.a & m.a) | (me.w.c & m.c) | (me.w.g & m.g) | (me.w.t & m.t));
				bits |= (uint32_t)(c >= sh.ol[o].floor2) << (o & 31);
			}
			sh.msk[wave][e][mw] = bits;
		}
	}
	wave_sync();
	if(!active[seq]) return;                                     // optimize.cpp:281
	const int32_t L = (int32_t)len[seq];
	const uint64_t base = blk_off[seq];
	for(uint32_t i = lane;i < run;i += 64){                       // k_pair
		const DevEntry me = ent[i];
		if(me.strand != 1) continue;
		for(uint32_t j = i + 1;j < run;++j){
			const DevEntry ej = ent[j];
			if(ej.loc - me.loc > amp_max + 128) break;
			if(ej.strand != 2) continue;
			for(uint32_t w = 0;w < mask_words;++w){
				const uint32_t mi = sh.msk[wave][i][w], mj = sh.msk[wave][j][w];
				uint32_t fr = mi & (mj >> 1) & 0x55555555u;
				uint32_t rf = (mi >> 1) & mj & 0x55555555u;
				uint32_t any = fr | rf;
				while(any){
					const uint32_t bit = __ffs(any) - 1;
					any &= any - 1;
					const uint32_t pair = (w*32 + bit) >> 1;
					if(pair >= n_pairs) break;
					const OligoDev F = sh.ol[2*pair], R = sh.ol[2*pair + 1];
					for(int orient = 0;orient < 2;++orient){
						if(!(((orient == 0) ? fr : rf) >> bit & 1u)) continue;
						const OligoDev &P = (orient == 0) ? F : R;
						const OligoDev &M = (orient == 0) ? R : F;
						if(me.loc + P.stop >= ej.loc - M.stop) continue;                     // pcr_assay.cpp:367-370
						int32_t amp_start = me.loc + P.start;
						const int32_t amp_stop = min(ej.loc - M.start, L - 1);
						int32_t amp_len = amp_stop - amp_start + 1;
						if(amp_len < amp_min || amp_len > amp_max) continue;
						if(amp_start < 0){ amp_len += amp_start; amp_start = 0; }
						if(amp_len < 0 || amp_start + amp_len > L){ atomicOr(&counters[1], 1u); continue; }
						if(has_split(planes, base, amp_start, amp_len)) continue;
						const float f = identity(F, (orient == 0) ? me.w : ej.w, use_taq);
						const float r = identity(R, (orient == 0) ? ej.w : me.w, use_taq);
						if(sqrtf(__fmul_rn(f, r)) >= ident_thr){                      // pcr_assay.cpp:572-576
							uint64_t *dst = (orient == 0) ? bits_fr : bits_rf;
							atomicOr((unsigned long long *)&dst[(size_t)pair*bit_words + (seq >> 6)], 1ull << (seq & 63));
						}
					}
				}
			}
		}
	}
}

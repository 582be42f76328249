// Cross-assay products of a primer pool (pcr_pool_products; included at the end of pcr_device.hip).
//
// Every ordered pair of distinct pool oligos (x, y) is asked what k_collect_amplicons answers for the pair (x, y) in
// orientation 0 (PCR::collect_unique_amplicons / extract_amplicon_seq, pcr_assay.cpp:443-542,756-813), over the word DB of
// the last select -- as a join over oligo hits, not one launch per combination:
//   1. k_pool_entry_oligos<false> / <true>: per DB slot, the distinct oligos its word matches at threshold^2 (count, scan,
//      fill: a CSR of (entry, oligo) items).  The oligo table sits in LDS; a thread tests its word against all of it.
//      Several DB entries can share a site (a regular and an irregular word at the same loc and strand): an oligo is listed
//      at the first of them only, so that every (oligo, site) is one item and every product one record.
//   2. k_pool_join<false> / <true>: one thread per item; a plus-strand item (i, x) walks the minus-strand items of its
//      sequence segment within amp_max + 128 of loc(i) (k_collect_amplicons' bound; entries are sorted by loc) and applies
//      the geometry (count, scan, emit at the scanned offsets).  The work is the hits' own: items x window items.
//   3. The records into (plus_oligo, minus_oligo, sequence, begin, end) order: a radix sort by (begin, end), a stable one
//      by (plus_oligo, minus_oligo, sequence), one gather that also sets `intended`.
// The call owns its scratch (pcr_ctx::pool_*): no buffer another entry point reads is written.
#include <map>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr uint32_t POOL_MAX_OLIGOS = 2*PCR_POOL_MAX_PAIRS;
constexpr int POOL_THREADS = 256;
constexpr uint64_t POOL_MAX_ITEMS = 1ull << 31;     // items and records are indexed by 32 bits

struct PoolOligo { Planes m; uint32_t floor2; int32_t start, stop; uint32_t pad; };   // fill_oligo's fields at threshold^2

__device__ __forceinline__ bool pool_hit(const Planes &w, const uint4 &m, uint32_t floor2)
{
	return (uint32_t)__popc((w.a & m.x) | (w.c & m.y) | (w.g & m.z) | (w.t & m.w)) >= floor2;
}

// DB thread g (db_slot's numbering) -> count[g] (<false>) or items[off[g] ..] = {g, oligo} (<true>).  Entries of inactive
// sequences list nothing: their plus sites make no product, and their minus sites pair only within the sequence.
template<bool FILL>
__global__ __launch_bounds__(POOL_THREADS) void k_pool_entry_oligos(const DevEntry *__restrict__ db, uint32_t n, uint32_t cap,
	const uint32_t *__restrict__ touched, const uint32_t *__restrict__ seg_hi, const uint8_t *__restrict__ active,
	const PoolOligo *__restrict__ oligos, uint32_t n_ol, uint32_t *__restrict__ count, const uint64_t *__restrict__ off,
	uint2 *__restrict__ items)
{
	__shared__ uint4 sm[POOL_MAX_OLIGOS];
	__shared__ uint32_t sf[POOL_MAX_OLIGOS];
	for(uint32_t o = threadIdx.x;o < n_ol;o += blockDim.x){
		const PoolOligo p = oligos[o];
		sm[o] = make_uint4(p.m.a, p.m.c, p.m.g, p.m.t); sf[o] = p.floor2;
	}
	__syncthreads();
	for(uint32_t g = blockIdx.x*blockDim.x + threadIdx.x;g < n;g += gridDim.x*blockDim.x){
		uint32_t slot, c = 0;
		if(db_slot(g, n, cap, touched, seg_hi, slot)){
			const DevEntry e = db[slot];
			if(active[e.seq] && (e.strand == 1 || e.strand == 2)){
				const uint32_t lo = e.seq*cap;
				const bool shared = slot > lo && db[slot - 1].loc == e.loc && db[slot - 1].strand == e.strand;
				uint64_t k = FILL ? off[g] : 0;
				for(uint32_t o = 0;o < n_ol;++o){
					if(!pool_hit(e.w, sm[o], sf[o])) continue;
					bool first = true;
					for(uint32_t p = slot;shared && p > lo;--p){
						const DevEntry q = db[p - 1];
						if(q.loc != e.loc || q.strand != e.strand) break;
						if(pool_hit(q.w, sm[o], sf[o])){ first = false; break; }
					}
					if(!first) continue;
					if(FILL) items[k++] = make_uint2(g, o);
					else ++c;
				}
			}
		}
		if(!FILL) count[g] = c;
	}
}

// One thread per item k: a plus-strand item (i, x) against the minus-strand items (j, y) of its segment; the tests of
// k_collect_amplicons for orientation 0 of the pair (x, y).  <false>: count[k]; <true>: records, (begin, end) sort keys and
// identity indices at rec_off[k] ..
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_pool_join(const DevEntry *__restrict__ db, uint32_t cap, const uint32_t *__restrict__ touched,
	const uint32_t *__restrict__ seg_hi, const uint2 *__restrict__ items, uint32_t n_items, const uint64_t *__restrict__ item_off,
	const PoolOligo *__restrict__ oligos, uint32_t n_ol, const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint64_t *__restrict__ len, const uint8_t *__restrict__ has_eos, int32_t amp_min, int32_t amp_max,
	uint32_t *__restrict__ count, const uint64_t *__restrict__ rec_off, pcr_product *__restrict__ rec, uint64_t *__restrict__ key,
	uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];                                        // Word::start() / stop()
	for(uint32_t o = threadIdx.x;o < n_ol;o += blockDim.x) ss[o] = make_int2(oligos[o].start, oligos[o].stop);
	__syncthreads();
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n_items) return;
	const uint2 it = items[k];
	const uint32_t g = it.x, x = it.y;
	const uint32_t i = touched[g/cap]*cap + g % cap;
	const DevEntry ei = db[i];
	uint32_t c = 0;
	uint64_t w = EMIT ? rec_off[k] : 0;
	if(ei.strand == 1){
		const uint32_t hi = seg_hi[ei.seq];
		const int32_t L = (int32_t)len[ei.seq];
		const uint64_t blk_base = blk_off[ei.seq];
		const bool eos = has_eos[ei.seq] != 0;
		const int2 P = ss[x];
		const int32_t p5 = ei.loc + P.x, p3 = ei.loc + P.y;                      // template_loc5/3, sequence.h:57-75
		for(uint32_t j = i + 1;j < hi;++j){
			const DevEntry ej = db[j];
			if(ej.loc - ei.loc > amp_max + 128) break;
			if(ej.strand != 2) continue;
			const uint32_t gj = g + (j - i);                                     // same segment: consecutive DB threads
			const uint64_t t_end = item_off[gj + 1];
			for(uint64_t t = item_off[gj];t < t_end;++t){
				const uint32_t y = items[t].y;
				const int2 M = ss[y];
				const int32_t m5 = ej.loc - M.y, m3 = ej.loc - M.x;
				if(p3 >= m5) continue;                                           // pcr_assay.cpp:468-471
				const int32_t amp_len = m3 - p5 + 1;
				if(amp_len < amp_min || amp_len > amp_max) continue;             // :477-484
				const int32_t in_start = p3 + 1 - 4;                             // :489-490
				const int32_t in_len = m5 - in_start + 8;                        // :492-494
				if(in_start < 0 || in_len < 0 || in_start + in_len > L) continue;
				if(eos && has_split(planes, blk_base, in_start, in_len)) continue;   // :504-521
				if(EMIT){
					pcr_product r;
					r.plus_oligo = x; r.minus_oligo = y; r.sequence = ei.seq; r.begin = p5; r.end = m3;
					r.inner_start = in_start; r.inner_length = in_len; r.intended = 0;
					rec[w] = r;
					key[w] = ((uint64_t)((uint32_t)p5 ^ 0x80000000u) << 32) | ((uint32_t)m3 ^ 0x80000000u);   // signed order
					ord[w] = (uint32_t)w;
					++w;
				}
				else ++c;
			}
		}
	}
	if(!EMIT) count[k] = c;
}

// (plus_oligo, minus_oligo, sequence) of the records in their (begin, end) order
__global__ void k_pool_key2(const pcr_product *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n, uint32_t seq_bits,
	uint32_t oligo_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	const pcr_product p = rec[ord[r]];
	key[r] = ((uint64_t)p.plus_oligo << (oligo_bits + seq_bits)) | ((uint64_t)p.minus_oligo << seq_bits) | p.sequence;
}

__global__ void k_pool_gather(const pcr_product *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n,
	const uint32_t *__restrict__ intended, uint32_t n_ol, pcr_product *__restrict__ out)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	pcr_product p = rec[ord[r]];
	const uint32_t b = p.plus_oligo*n_ol + p.minus_oligo;
	p.intended = (intended[b >> 5] >> (b & 31)) & 1u;
	out[r] = p;
}

unsigned pool_bits(uint64_t n) { unsigned b = 1; while(b < 32 && (1ull << b) < n) ++b; return b; }

} // namespace

extern "C" {

int64_t pcr_pool_products(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, uint32_t *oligo_id, pcr_product *out, uint64_t cap)
{
	static_assert(sizeof(pcr_product) == 32, "record layout");
	static_assert(sizeof(PoolOligo) == 32, "oligo layout");
	if(!set_ok(which)){ g_err = "pcr_pool_products: unknown sequence set"; return PCR_ERR_ARG; }
	if(!ctx || (which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND) || (n_pool && (!pool || !oligo_id)) || (cap && !out)){
		g_err = "pcr_pool_products: bad argument"; return PCR_ERR_ARG;
	}
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = "pcr_pool_products: pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = "pcr_pool_products: no word DB (call pcr_select_words first)"; return PCR_ERR_STATE; }
	if(n_pool == 0) return 0;
	// the distinct oligos, in order of first appearance
	std::vector<PoolOligo> ol;
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> id_of;
	const float thr2 = threshold*threshold;                                      // pcr_assay.cpp:775-776
	for(uint32_t s = 0;s < 2*n_pool;++s){
		const pcr_word128 &wd = (s & 1) ? pool[s/2].r : pool[s/2].f;
		auto ins = id_of.insert(std::make_pair(std::make_pair(wd.w[0], wd.w[1]), (uint32_t)ol.size()));
		if(ins.second){
			OligoDev d; fill_oligo(d, wd.w, thr2);
			PoolOligo p; p.m = d.m; p.floor2 = d.floor2; p.start = d.start; p.stop = d.stop; p.pad = 0;
			ol.push_back(p);
		}
		oligo_id[s] = ins.first->second;
	}
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	if(S.n_entries == 0 || S.n_touched == 0) return 0;
	const uint32_t n_ol = (uint32_t)ol.size();
	std::vector<uint32_t> intended(((size_t)n_ol*n_ol + 31)/32, 0);
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		for(uint32_t b : {f*n_ol + r, r*n_ol + f}) intended[b >> 5] |= 1u << (b & 31);
	}
	int rc;
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo);
	if((rc = ctx->pool_in.ensure(ol_bytes + intended.size()*sizeof(uint32_t))) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)ctx->pool_in.p;
	const uint32_t *d_intended = (const uint32_t *)(ctx->pool_in.p + ol_bytes);
	HIP_TRY(hipMemcpyAsync(ctx->pool_in.p, ol.data(), ol_bytes, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemcpyAsync(ctx->pool_in.p + ol_bytes, intended.data(), intended.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
	// ---- 1. per-entry oligo lists
	const uint32_t n_db = S.n_touched*S.db_cap;
	if((rc = ctx->pool_cnt.ensure((size_t)n_db + 1)) != PCR_OK) return rc;
	if((rc = ctx->pool_eoff.ensure((size_t)n_db + 1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->pool_cnt.p + n_db, 0, sizeof(uint32_t), ctx->stream));
	size_t tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->pool_cnt.p, ctx->pool_eoff.p, uint64_t(0), (size_t)n_db + 1, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->pool_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	const unsigned grid_e = std::min<unsigned>((n_db + POOL_THREADS - 1)/POOL_THREADS, ctx->n_cu*8);
	hipLaunchKernelGGL(k_pool_entry_oligos<false>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, ctx->pool_cnt.p, (const uint64_t *)nullptr, (uint2 *)nullptr);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::exclusive_scan(ctx->pool_tmp.p, tmp, ctx->pool_cnt.p, ctx->pool_eoff.p, uint64_t(0), (size_t)n_db + 1, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t n_items = 0;
	HIP_TRY(hipMemcpyAsync(&n_items, ctx->pool_eoff.p + n_db, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products: too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0) return 0;
	if((rc = ctx->pool_items.ensure(n_items)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_pool_entry_oligos<true>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, (uint32_t *)nullptr, (const uint64_t *)ctx->pool_eoff.p, ctx->pool_items.p);
	HIP_TRY(hipGetLastError());
	// ---- 2. the join: count, scan
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->pool_cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;       // (the entry counts are spent)
	if((rc = ctx->pool_ioff.ensure((size_t)ni + 1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->pool_cnt.p + ni, 0, sizeof(uint32_t), ctx->stream));
	hipLaunchKernelGGL(k_pool_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		ctx->pool_items.p, ni, (const uint64_t *)ctx->pool_eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_has_eos.p,
		amp_min, amp_max, ctx->pool_cnt.p, (const uint64_t *)nullptr, (pcr_product *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	tmp = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, ctx->pool_cnt.p, ctx->pool_ioff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->pool_tmp.ensure(tmp + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::exclusive_scan(ctx->pool_tmp.p, tmp, ctx->pool_cnt.p, ctx->pool_ioff.p, uint64_t(0), (size_t)ni + 1, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, ctx->pool_ioff.p + ni, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(total >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products: too many products"; return PCR_ERR_CAPACITY; }
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 2'. emit at the scanned offsets; 3. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->pool_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pool_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pool_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_product *r0 = ctx->pool_rec.p, *r1 = r0 + nr;
	uint64_t *k0 = ctx->pool_keys.p, *k1 = k0 + nr;
	uint32_t *o0 = ctx->pool_ord.p, *o1 = o0 + nr;
	hipLaunchKernelGGL(k_pool_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, S.db_cap, S.touched.p, S.d_seg_hi,
		ctx->pool_items.p, ni, (const uint64_t *)ctx->pool_eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p, S.d_has_eos.p,
		amp_min, amp_max, (uint32_t *)nullptr, (const uint64_t *)ctx->pool_ioff.p, r0, k0, o0);
	HIP_TRY(hipGetLastError());
	const unsigned seq_bits = pool_bits(S.n), oligo_bits = pool_bits(n_ol);
	size_t t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));
	if((rc = ctx->pool_tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->pool_tmp.p, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	const unsigned grid_r = (nr + 255)/256;
	hipLaunchKernelGGL(k_pool_key2, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_product *)r0, (const uint32_t *)o1, nr, seq_bits, oligo_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(ctx->pool_tmp.p, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_pool_gather, dim3(grid_r), dim3(256), 0, ctx->stream, (const pcr_product *)r0, (const uint32_t *)o0, nr, d_intended, n_ol, r1);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_product), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // extern "C"

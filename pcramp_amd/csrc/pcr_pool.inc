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
//      sequence segment near loc(i) and applies the geometry (join_walk; count, scan, emit at the scanned offsets).  The
//      work is the hits' own: items x window items.
//   3. The records into (plus_oligo, minus_oligo, sequence, begin, end) order (product_order).
// The call owns its scratch (pcr_ctx::pool_*): no buffer another entry point reads is written.
// The entry points built on the same items share this file's stages: scan_total, item_count / item_fill, join_walk (the one
// place the amplicon geometry is written), product_order.
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

// cnt[0 .. n) -> off[0 .. n], their exclusive sums, and total = off[n].  cnt has n + 1 elements; the last is zeroed here.
// Synchronous: everything queued on the stream before the call has run when it returns.  more(): what the caller copies back
// on the same wait (its flags, its bit rows); it returns PCR_OK or an error.  It is a functor because of where it must run:
// behind the total's copy.  A copy to pageable memory makes the host wait for the stream, so one queued before the scan would
// keep the scan's launches from being issued while the kernel before them runs.
template<class O, class More>
int scan_total(pcr_ctx *ctx, uint32_t *cnt, DevBuf<O> &off, DevBuf<uint8_t> &tmp, size_t n, O &total, More &&more)
{
	int rc;
	if((rc = off.ensure(n + 1)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(cnt + n, 0, sizeof(uint32_t), ctx->stream));
	size_t bytes = 0;
	HIP_TRY(rocprim::exclusive_scan(nullptr, bytes, cnt, off.p, O(0), n + 1, rocprim::plus<O>(), ctx->stream));
	if((rc = tmp.ensure(bytes + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::exclusive_scan(tmp.p, bytes, cnt, off.p, O(0), n + 1, rocprim::plus<O>(), ctx->stream));
	total = 0;
	HIP_TRY(hipMemcpyAsync(&total, off.p + n, sizeof(O), hipMemcpyDeviceToHost, ctx->stream));
	if((rc = more()) != PCR_OK) return rc;
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return PCR_OK;
}
template<class O>
int scan_total(pcr_ctx *ctx, uint32_t *cnt, DevBuf<O> &off, DevBuf<uint8_t> &tmp, size_t n, O &total)
{
	return scan_total(ctx, cnt, off, tmp, n, total, []{ return (int)PCR_OK; });
}

// The item stage, in two phases because callers act between them (a count above cap ends pcr_site_tm before any fill).
// item_count: the per-entry counts and B.eoff, their scan -> n_items (synchronous; the "too many" refusal is the caller's, in its
// words).  item_fill: B.items[0 .. n_items), with n_items > 0 what item_count gave for the same oligo table.
int item_count(pcr_ctx *ctx, const SeqSet &S, const PoolOligo *d_ol, uint32_t n_ol, const ItemBufs &B, uint64_t &n_items)
{
	int rc;
	const uint32_t n_db = S.n_touched*S.db_cap;
	if((rc = B.cnt->ensure((size_t)n_db + 1)) != PCR_OK) return rc;
	const unsigned grid_e = std::min<unsigned>((n_db + POOL_THREADS - 1)/POOL_THREADS, ctx->n_cu*8);
	hipLaunchKernelGGL(k_pool_entry_oligos<false>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, B.cnt->p, (const uint64_t *)nullptr, (uint2 *)nullptr);
	HIP_TRY(hipGetLastError());
	return scan_total(ctx, B.cnt->p, *B.eoff, *B.tmp, n_db, n_items);
}

int item_fill(pcr_ctx *ctx, const SeqSet &S, const PoolOligo *d_ol, uint32_t n_ol, const ItemBufs &B, uint64_t n_items)
{
	int rc;
	const uint32_t n_db = S.n_touched*S.db_cap;
	if((rc = B.items->ensure(n_items)) != PCR_OK) return rc;
	const unsigned grid_e = std::min<unsigned>((n_db + POOL_THREADS - 1)/POOL_THREADS, ctx->n_cu*8);
	hipLaunchKernelGGL(k_pool_entry_oligos<true>, dim3(grid_e), dim3(POOL_THREADS), 0, ctx->stream, S.db.p, n_db, S.db_cap, S.touched.p,
		S.d_seg_hi, S.d_active.p, d_ol, n_ol, (uint32_t *)nullptr, (const uint64_t *)B.eoff->p, B.items->p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// What a join kernel reads of the word DB and its sequences, the items, and the amplicon length bounds.
struct JoinIn {
	const DevEntry *__restrict__ db; uint32_t cap; const uint32_t *__restrict__ touched; const uint32_t *__restrict__ seg_hi;
	const uint2 *__restrict__ items; uint32_t n_items; const uint64_t *__restrict__ item_off;
	const PoolOligo *__restrict__ oligos; uint32_t n_ol; const uint4 *__restrict__ planes; const uint64_t *__restrict__ blk_off;
	const uint64_t *__restrict__ len; const uint8_t *__restrict__ has_eos; int32_t amp_min, amp_max;
};

// Word::start() / stop() of the oligos into LDS (POOL_MAX_OLIGOS of them), for join_walk
__device__ __forceinline__ void join_geometry(const JoinIn &J, int2 *ss)
{
	for(uint32_t o = threadIdx.x;o < J.n_ol;o += blockDim.x) ss[o] = make_int2(J.oligos[o].start, J.oligos[o].stop);
	__syncthreads();
}

// The walk of every join kernel: the plus-strand item (i, x) of DB thread g, ei = db[i], against the minus-strand items (j, y)
// -- with MINUS_BELOW only those with y < n_minus (k_probe_products: a probe takes no primer role) -- of its segment within k_collect_amplicons' bound of loc(i) (entries are sorted by loc), under the
// tests of k_collect_amplicons for orientation 0 of the pair (x, y), in the reference's order.  Every survivor:
// keep(t, y, j, p5, m3, in_start, in_len), t the minus item's index.  It does not return from the kernel.
template<bool MINUS_BELOW, class F>
__device__ __forceinline__ void join_walk(const JoinIn &J, const int2 *ss, uint32_t g, uint32_t x, uint32_t i, const DevEntry &ei, uint32_t n_minus, F &&keep)
{
	const uint32_t hi = J.seg_hi[ei.seq];
	const int32_t L = (int32_t)J.len[ei.seq];
	const uint64_t blk_base = J.blk_off[ei.seq];
	const bool eos = J.has_eos[ei.seq] != 0;
	const int2 P = ss[x];
	const int32_t p5 = ei.loc + P.x, p3 = ei.loc + P.y;                          // template_loc5/3, sequence.h:57-75
	for(uint32_t j = i + 1;j < hi;++j){
		const DevEntry ej = J.db[j];
		if(ej.loc - ei.loc > J.amp_max + 128) break;
		if(ej.strand != 2) continue;
		const uint32_t gj = g + (j - i);                                         // same segment: consecutive DB threads
		const uint64_t t_end = J.item_off[gj + 1];
		for(uint64_t t = J.item_off[gj];t < t_end;++t){
			const uint32_t y = J.items[t].y;
			if(MINUS_BELOW && y >= n_minus) continue;
			const int2 M = ss[y];
			const int32_t m5 = ej.loc - M.y, m3 = ej.loc - M.x;
			if(p3 >= m5) continue;                                               // pcr_assay.cpp:468-471
			const int32_t amp_len = m3 - p5 + 1;
			if(amp_len < J.amp_min || amp_len > J.amp_max) continue;             // :477-484
			const int32_t in_start = p3 + 1 - 4;                                 // :489-490
			const int32_t in_len = m5 - in_start + 8;                            // :492-494
			if(in_start < 0 || in_len < 0 || in_start + in_len > L) continue;
			if(eos && has_split(J.planes, blk_base, in_start, in_len)) continue;   // :504-521
			keep(t, y, j, p5, m3, in_start, in_len);
		}
	}
}

__device__ __forceinline__ uint64_t product_key1(int32_t begin, int32_t end)    // (begin, end) in signed order
{
	return ((uint64_t)((uint32_t)begin ^ 0x80000000u) << 32) | ((uint32_t)end ^ 0x80000000u);
}

// One thread per item k: join_walk; <false>: count[k]; <true>: records, (begin, end) sort keys and identity indices at rec_off[k] ..
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_pool_join(const JoinIn J, uint32_t *__restrict__ count, const uint64_t *__restrict__ rec_off,
	pcr_product *__restrict__ rec, uint64_t *__restrict__ key, uint32_t *__restrict__ ord)
{
	__shared__ int2 ss[POOL_MAX_OLIGOS];
	join_geometry(J, ss);
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= J.n_items) return;
	const uint2 it = J.items[k];
	const uint32_t g = it.x, x = it.y;
	const uint32_t i = J.touched[g/J.cap]*J.cap + g % J.cap;
	const DevEntry ei = J.db[i];
	uint32_t c = 0;
	uint64_t w = EMIT ? rec_off[k] : 0;
	if(ei.strand == 1) join_walk<false>(J, ss, g, x, i, ei, 0u, [&](uint64_t, uint32_t y, uint32_t, int32_t p5, int32_t m3, int32_t in_start, int32_t in_len){
		if(EMIT){
			pcr_product r;
			r.plus_oligo = x; r.minus_oligo = y; r.sequence = ei.seq; r.begin = p5; r.end = m3;
			r.inner_start = in_start; r.inner_length = in_len; r.intended = 0;
			rec[w] = r;
			key[w] = product_key1(p5, m3);
			ord[w] = (uint32_t)w;
			++w;
		}
		else ++c;
	});
	if(!EMIT) count[k] = c;
}

// (plus_oligo, minus_oligo, sequence) of the records (pcr_product or pcr_product_tm) in their (begin, end) order
template<class R>
__global__ void k_product_key2(const R *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n, uint32_t seq_bits,
	uint32_t oligo_bits, uint64_t *__restrict__ key)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	const uint32_t at = ord[r];
	const uint32_t plus = rec[at].plus_oligo, minus = rec[at].minus_oligo, seq = rec[at].sequence;
	key[r] = ((uint64_t)plus << (oligo_bits + seq_bits)) | ((uint64_t)minus << seq_bits) | seq;
}

template<class R>
__global__ void k_product_gather(const R *__restrict__ rec, const uint32_t *__restrict__ ord, uint32_t n,
	const uint32_t *__restrict__ intended, uint32_t n_ol, R *__restrict__ out)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r >= n) return;
	R p = rec[ord[r]];
	const uint32_t b = p.plus_oligo*n_ol + p.minus_oligo;
	p.intended = (intended[b >> 5] >> (b & 31)) & 1u;
	out[r] = p;
}

unsigned pool_bits(uint64_t n) { unsigned b = 1; while(b < 32 && (1ull << b) < n) ++b; return b; }

// The record order of products: the nr records r0[] with their (begin, end) keys k0[] and identity indices o0[] (each buffer holds
// 2*nr) into (plus_oligo, minus_oligo, sequence, begin, end) order at r0 + nr, `intended` set -- a radix sort by (begin, end), a
// stable one by (plus_oligo, minus_oligo, sequence), one gather.  Queued on the stream; the caller copies out and waits.
template<class R>
int product_order(pcr_ctx *ctx, R *r0, uint64_t *k0, uint32_t *o0, uint32_t nr, unsigned seq_bits, unsigned oligo_bits,
	const uint32_t *d_intended, uint32_t n_ol, DevBuf<uint8_t> &tmp)
{
	int rc;
	uint64_t *k1 = k0 + nr;
	uint32_t *o1 = o0 + nr;
	size_t t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));
	if((rc = tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(tmp.p, t1, k0, k1, o0, o1, nr, 0, 64, ctx->stream));
	const unsigned grid_r = (nr + 255)/256;
	hipLaunchKernelGGL(k_product_key2<R>, dim3(grid_r), dim3(256), 0, ctx->stream, (const R *)r0, (const uint32_t *)o1, nr, seq_bits, oligo_bits, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::radix_sort_pairs(tmp.p, t2, k0, k1, o1, o0, nr, 0, 2*oligo_bits + seq_bits, ctx->stream));   // (stable)
	hipLaunchKernelGGL(k_product_gather<R>, dim3(grid_r), dim3(256), 0, ctx->stream, (const R *)r0, (const uint32_t *)o0, nr, d_intended, n_ol, r0 + nr);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

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
	const ItemBufs B{&ctx->pool_tmp, &ctx->pool_cnt, &ctx->pool_eoff, &ctx->pool_items};
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products: too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0) return 0;
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	// ---- 2. the join: count, scan
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = ctx->pool_cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;       // (the entry counts are spent)
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, ctx->pool_items.p, ni, ctx->pool_eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p,
		S.d_len.p, S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_pool_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, ctx->pool_cnt.p, (const uint64_t *)nullptr,
		(pcr_product *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	uint64_t total = 0;
	if((rc = scan_total(ctx, ctx->pool_cnt.p, ctx->pool_ioff, ctx->pool_tmp, ni, total)) != PCR_OK) return rc;
	if(total >= POOL_MAX_ITEMS){ g_err = "pcr_pool_products: too many products"; return PCR_ERR_CAPACITY; }
	if(total == 0 || total > cap) return (int64_t)total;                         // count only: out is left as it is
	// ---- 2'. emit at the scanned offsets; 3. the key order
	const uint32_t nr = (uint32_t)total;
	if((rc = ctx->pool_rec.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pool_keys.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	if((rc = ctx->pool_ord.ensure(2*(size_t)nr)) != PCR_OK) return rc;
	pcr_product *r0 = ctx->pool_rec.p, *r1 = r0 + nr;
	hipLaunchKernelGGL(k_pool_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, (uint32_t *)nullptr, (const uint64_t *)ctx->pool_ioff.p,
		r0, ctx->pool_keys.p, ctx->pool_ord.p);
	HIP_TRY(hipGetLastError());
	if((rc = product_order(ctx, r0, ctx->pool_keys.p, ctx->pool_ord.p, nr, pool_bits(S.n), pool_bits(n_ol), d_intended, n_ol, ctx->pool_tmp)) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(out, r1, (size_t)nr*sizeof(pcr_product), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)total;
}

} // extern "C"

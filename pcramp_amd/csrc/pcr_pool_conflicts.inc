// Which assays of a primer pool cannot share a tube: the pool's spurious products and its oligo-by-oligo dimers reduced to
// unordered pairs of pool rows on the device (pcr_pool_conflicts; included by pcr_device.hip after pcr_pool.inc and pcr_site_tm.inc,
// whose stages are its steps 1-3, and after pcr_pool_dimers.inc, whose plan and kernels it runs).
//
// A spurious product (plus oligo x, minus oligo y) belongs to every unordered row pair {i, j} with (x in O(i), y in O(j)) or
// (x in O(j), y in O(i)): the unordered pairs of rows(x) x rows(y).  The ordered walk meets {i, j} twice exactly when (j, i) is
// in rows(x) x rows(y) as well; the copy with i > j is dropped then, which needs the two rows' oligo ids and no memory.
//   1-3. the items, the jobs, k_site_tm, k_item_tm -> item_tm[] (item_count / item_fill, melt_items, on the shared scratch set).
//   4. k_conflict_join<false> / <true>: k_products_join's walk (join_walk) with the floor; a kept product that is no pool pair's
//      walks rows(x) x rows(y).  Count pass, scan, emit pass: one (cell << seq_bits | sequence, bits of v) pair per attribution.
//   5. rocprim::radix_sort_pairs by (cell, sequence), then rocprim::reduce_by_key over the cells with {max of (v bits << 32 |
//      ~sequence), count, count of (cell, sequence) run heads}: products, sequences, melt and melt_sequence of every cell with a
//      product.  v >= +0 (v + 0.0f), so the floats order like their bits; every operand is an integer and the operator is
//      associative and commutative: the bytes do not depend on the order the device works in, and no atomic is made.  A cell fed
//      by every product of a large family is a long run of the sorted keys, reduced like any other run.
//   6. k_conflict_scatter puts the aggregates into a dense array over the n_pool(n_pool + 1)/2 cells.
//   7. With a dimer rule: pcr_pool_dimers' plan, k_pool_dimer and k_pool_dimer_reduce batch by batch as they stand;
//      k_conflict_dimer_store keeps tm_max of every cell in a dense n_ol x n_ol matrix on the device.
//   8. k_conflict_cells: a thread per cell a <= b joins the aggregate with the maximum of the cell's (up to eight) dimer cells,
//      the lowest (q, t) on a tie, and sets the flags and the keep word; an exclusive scan and k_conflict_compact put the kept
//      cells into (row_a, row_b) order.
// Steps 1-4 work in pcr_ctx::shared (its flag holds two words here), the rest in pcr_ctx::pcf_*; the dG table is the handle's (th_dg, keyed by its salt).
// pcr_pool_conflicts_end3 is the same call with a 3'-end rule (pcr_products_end3.inc, included before this file) on the products
// of steps 1-6: k_item_end3 fills an ItemEnd per item before the melt, and the join's functor makes k_end3_join's tests behind
// the floor.  Steps 7 and 8 do not know the rule.
// pcr_pool_conflicts_ext (pcr_pool_conflicts_ext.inc, included after this file) is pool_conflicts_impl as well: with a ConflictExt
// the arguments of ext are checked behind the rule's, and after step 8 conflict_ext_tail takes over from pcf_rec and pcf_keep.

#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr uint32_t PCF_CELL_BITS = 20;
static_assert((uint64_t)PCR_POOL_MAX_PAIRS*(PCR_POOL_MAX_PAIRS + 1)/2 <= (1ull << PCF_CELL_BITS), "a cell index fits PCF_CELL_BITS");
constexpr uint64_t PCF_MAX_ATTRIBUTIONS = 1ull << 31;

// what the cells of a run of attributions reduce to: best = bits of v << 32 | ~sequence (the highest v, then the lowest sequence)
struct alignas(16) ConflictAgg { unsigned long long best; uint32_t products, sequences; };

// the index of the unordered row pair a <= b among the n(n + 1)/2 cells, in (a, b) order
__host__ __device__ inline uint32_t pcf_cell(uint32_t a, uint32_t b, uint32_t n) { return a*n - (a*(a - 1u))/2u + (b - a); }

struct PcfCellOf {
	uint32_t shift;
	__host__ __device__ uint32_t operator()(const uint64_t &k) const { return (uint32_t)(k >> shift); }
};
struct PcfAggOf {
	const uint64_t *key; const uint32_t *val; uint64_t seq_mask;
	__host__ __device__ ConflictAgg operator()(const uint32_t &i) const
	{
		const uint64_t k = key[i];
		ConflictAgg a;
		a.best = ((unsigned long long)val[i] << 32) | (uint32_t)~(uint32_t)(k & seq_mask);
		a.products = 1u;
		a.sequences = (i == 0u || key[i - 1u] != k) ? 1u : 0u;                      // the first attribution of its (cell, sequence)
		return a;
	}
};
struct PcfMerge {
	__host__ __device__ ConflictAgg operator()(const ConflictAgg &a, const ConflictAgg &b) const
	{
		ConflictAgg r;
		r.best = (a.best > b.best) ? a.best : b.best;
		r.products = a.products + b.products;
		r.sequences = a.sequences + b.sequences;
		return r;
	}
};

// k_products_join with the floor, over the spurious kept products only: one thread per item k, join_walk.  Every attribution of a
// product to a cell: <false> counts it, <true> writes its key and the bits of v at att_off[k] ..  item_end != NULL: only the
// products that also pass the 3'-end rule R (k_end3_join's tests, after the floor).
template<bool EMIT>
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_join(const JoinIn J, const ItemTm *__restrict__ item_tm, float tm_floor,
	const ItemEnd *__restrict__ item_end, const End3Rule R, const uint32_t *__restrict__ intended, const uint32_t *__restrict__ rows_off, const uint32_t *__restrict__ rows, const uint2 *__restrict__ row_ol,
	uint32_t n_pool, uint32_t seq_bits, uint32_t *__restrict__ count, const uint64_t *__restrict__ att_off, uint64_t *__restrict__ key,
	uint32_t *__restrict__ val)
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
	uint64_t w = EMIT ? att_off[k] : 0;
	if(ei.strand == 1){
		const ItemTm tp = item_tm[k];
		const bool floored = tm_floor > 0.0f;
		const uint32_t x0 = rows_off[x], x1 = rows_off[x + 1];
		ItemEnd ep; ep.clamp3 = ep.end_mismatch = ep.length = ep.pad = 0; ep.id = 0.0f;
		if(item_end) ep = item_end[k];
		const bool plus_ok = !item_end || end3_site_ok(ep, R);
		auto keep = [&](uint64_t t, uint32_t y, uint32_t, int32_t, int32_t, int32_t, int32_t){
			const uint32_t b = x*J.n_ol + y;
			if((intended[b >> 5] >> (b & 31)) & 1u) return;                      // a pool pair's own product is no conflict
			const ItemTm tm = item_tm[t];
			const float v = ((tp.tm < tm.tm) ? tp.tm : tm.tm) + 0.0f;            // k_products_join's min; + 0.0f: -0 -> +0 (contraction is off)
			if(floored && !(v >= tm_floor)) return;
			ItemEnd em;
			if(item_end && !end3_product_ok(item_end, R, plus_ok, ep, t, em)) return;
			const uint32_t y0 = rows_off[y], y1 = rows_off[y + 1];
			for(uint32_t ia = x0;ia < x1;++ia){
				const uint32_t ri = rows[ia];
				for(uint32_t ja = y0;ja < y1;++ja){
					const uint32_t rj = rows[ja];
					if(ri > rj){
						// {rj, ri} arises again as (rj in rows(x), ri in rows(y)): that copy, with the lower row first, is the one kept
						const uint2 oj = row_ol[rj], oi = row_ol[ri];
						if((oj.x == x || oj.y == x) && (oi.x == y || oi.y == y)) continue;
					}
					if(EMIT){
						const uint32_t cell = (ri <= rj) ? pcf_cell(ri, rj, n_pool) : pcf_cell(rj, ri, n_pool);
						key[w] = ((uint64_t)cell << seq_bits) | ei.seq;
						val[w] = __float_as_uint(v);
						++w;
					}
					else ++c;
				}
			}
		};
		// (a plus site below the floor keeps no product, nor does one that fails its own half of the rule)
		if(!(floored && tp.tm < tm_floor) && plus_ok) join_walk<false>(J, ss, g, x, i, ei, 0u, keep);
	}
	if(!EMIT) count[k] = c;
}

// the aggregates of the cells that have a product -> their places in the dense array (zero elsewhere)
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_scatter(const uint32_t *__restrict__ ucell, const ConflictAgg *__restrict__ uagg,
	const uint32_t *__restrict__ n_unique, uint32_t n_cells, ConflictAgg *__restrict__ dense)
{
	const uint32_t n = *n_unique;
	for(uint32_t u = blockIdx.x*blockDim.x + threadIdx.x;u < n;u += gridDim.x*blockDim.x){
		const uint32_t c = ucell[u];
		if(c < n_cells) dense[c] = uagg[u];
	}
}

// tm_max of a batch's cells c0 .. c0 + n_cells - 1 (c = q*n_ol + t) into the dense matrix
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_dimer_store(const pcr_pool_dimer *__restrict__ rec, uint32_t n_cells, float *__restrict__ mat)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells) mat[k] = rec[k].tm_max;
}

// Cell {a, b}, a = blockIdx.y <= b: the record and its keep word.  dmat = NULL: no dimers were asked for.
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_cells(const ConflictAgg *__restrict__ dense, const float *__restrict__ dmat, uint32_t n_ol,
	const uint2 *__restrict__ row_ol, uint32_t n_pool, float dimer_floor, pcr_pool_conflict *__restrict__ rec, uint32_t *__restrict__ keep)
{
	const uint32_t a = blockIdx.y, b = blockIdx.x*blockDim.x + threadIdx.x;
	if(b >= n_pool || b < a) return;
	const uint32_t c = pcf_cell(a, b, n_pool);
	const ConflictAgg g = dense[c];
	pcr_pool_conflict r;
	r.row_a = a; r.row_b = b;
	r.products = g.products; r.sequences = g.sequences;
	r.melt = g.products ? __uint_as_float((uint32_t)(g.best >> 32)) : PCR_ANNEAL_NO_PRODUCT;
	r.melt_sequence = g.products ? ~(uint32_t)g.best : 0u;
	r.dimer_tm = 0.0f; r.dimer_query = r.dimer_target = 0u;
	r.flags = g.products ? PCR_CONFLICT_PRODUCT : 0u;
	r.reserved = 0u;
	bool kept = g.products != 0u;
	if(dmat){
		const uint2 oa = row_ol[a], ob = row_ol[b];
		// the (up to eight) ordered cells as q*n_ol + t, ascending: the first of the highest values is the lowest (q, t) on a tie
		uint32_t cell[8] = {oa.x*n_ol + ob.x, oa.x*n_ol + ob.y, oa.y*n_ol + ob.x, oa.y*n_ol + ob.y,
			ob.x*n_ol + oa.x, ob.y*n_ol + oa.x, ob.x*n_ol + oa.y, ob.y*n_ol + oa.y};
		for(int i = 1;i < 8;++i){
			for(int j = i;j > 0 && cell[j - 1] > cell[j];--j){ const uint32_t s = cell[j]; cell[j] = cell[j - 1]; cell[j - 1] = s; }
		}
		for(int i = 0;i < 8;++i){
			const float tm = dmat[cell[i]];
			if(i == 0 || tm > r.dimer_tm){ r.dimer_tm = tm; r.dimer_query = cell[i]/n_ol; r.dimer_target = cell[i] % n_ol; }
		}
		if(r.dimer_tm >= dimer_floor) r.flags |= PCR_CONFLICT_DIMER;
		if(!(dimer_floor > 0.0f) || r.dimer_tm >= dimer_floor) kept = true;
	}
	rec[c] = r;
	keep[c] = kept ? 1u : 0u;
}

// the kept cells, in cell order: off = exclusive scan of keep
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_compact(const pcr_pool_conflict *__restrict__ rec, const uint32_t *__restrict__ keep,
	const uint32_t *__restrict__ off, uint32_t n_cells, pcr_pool_conflict *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells && keep[k]) out[off[k]] = rec[k];
}

// Steps 1-6: the aggregates of the spurious kept products in ctx->pcf_dense[0 .. n_cells) (zero where a cell has none).
// ruled: the products must pass R as well (the 3' end per item: pcr_pool_products_end3's step 2, before the melt).
int conflict_products(const std::string &who, pcr_ctx *ctx, SeqSet &S, const std::vector<PoolOligo> &ol, const std::vector<SiteOligoX> &olx, const uint32_t *oligo_id,
	uint32_t n_pool, int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float tm_floor, const End3Rule &R, bool ruled, int use_taq,
	uint32_t n_cells)
{
	int rc;
	const uint32_t n_ol = (uint32_t)ol.size();
	// the intended bitmap; the rows of every distinct oligo (a row with F = R once); each row's two oligos
	std::vector<uint32_t> intended(((size_t)n_ol*n_ol + 31)/32, 0), rows_off(n_ol + 1, 0), rows;
	std::vector<uint2> row_ol(n_pool);
	for(uint32_t i = 0;i < n_pool;++i){
		const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
		for(uint32_t b : {f*n_ol + r, r*n_ol + f}) intended[b >> 5] |= 1u << (b & 31);
		row_ol[i] = make_uint2(f, r);
		++rows_off[f + 1];
		if(r != f) ++rows_off[r + 1];
	}
	for(uint32_t o = 0;o < n_ol;++o) rows_off[o + 1] += rows_off[o];
	rows.resize(rows_off[n_ol]);
	{
		std::vector<uint32_t> at(rows_off.begin(), rows_off.end() - 1);
		for(uint32_t i = 0;i < n_pool;++i){                                       // (ascending rows within an oligo)
			const uint32_t f = oligo_id[2*i], r = oligo_id[2*i + 1];
			rows[at[f]++] = i;
			if(r != f) rows[at[r]++] = i;
		}
	}
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), olx_bytes = olx.size()*sizeof(SiteOligoX), rol_bytes = row_ol.size()*sizeof(uint2),
		int_bytes = intended.size()*sizeof(uint32_t), off_bytes = rows_off.size()*sizeof(uint32_t), rows_bytes = rows.size()*sizeof(uint32_t);
	const std::vector<float> norm = ruled ? end3_norms(ol) : std::vector<float>();   // (k_item_end3's; only a rule reads it)
	const size_t norm_bytes = norm.size()*sizeof(float);
	std::vector<uint8_t> blob(ol_bytes + olx_bytes + rol_bytes + int_bytes + off_bytes + rows_bytes + norm_bytes);   // 32-, 8-, 8-, 4-, 4-, 4- and 4-byte records, in that order: each is aligned
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, olx.data(), olx_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes, row_ol.data(), rol_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + rol_bytes, intended.data(), int_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + rol_bytes + int_bytes, rows_off.data(), off_bytes);
	memcpy(blob.data() + ol_bytes + olx_bytes + rol_bytes + int_bytes + off_bytes, rows.data(), rows_bytes);
	if(norm_bytes) memcpy(blob.data() + ol_bytes + olx_bytes + rol_bytes + int_bytes + off_bytes + rows_bytes, norm.data(), norm_bytes);
	ItemScratch &X = ctx->shared;
	const ItemBufs B = X.bufs();
	if((rc = X.in.ensure(blob.size())) != PCR_OK) return rc;
	const PoolOligo *d_ol = (const PoolOligo *)X.in.p;
	const SiteOligoX *d_olx = (const SiteOligoX *)(X.in.p + ol_bytes);
	const uint2 *d_row_ol = (const uint2 *)(X.in.p + ol_bytes + olx_bytes);
	const uint32_t *d_intended = (const uint32_t *)(X.in.p + ol_bytes + olx_bytes + rol_bytes);
	const uint32_t *d_rows_off = (const uint32_t *)(X.in.p + ol_bytes + olx_bytes + rol_bytes + int_bytes);
	const uint32_t *d_rows = (const uint32_t *)(X.in.p + ol_bytes + olx_bytes + rol_bytes + int_bytes + off_bytes);
	const float *d_norm = (const float *)(X.in.p + ol_bytes + olx_bytes + rol_bytes + int_bytes + off_bytes + rows_bytes);
	HIP_TRY(hipMemcpyAsync(X.in.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));                                   // (blob is this function's)
	if(S.n_entries == 0 || S.n_touched == 0) return PCR_OK;
	// ---- 1. the items
	uint64_t n_items = 0;
	if((rc = item_count(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	if(n_items >= POOL_MAX_ITEMS){ g_err = who + ": too many (entry, oligo) hits"; return PCR_ERR_CAPACITY; }
	if(n_items == 0) return PCR_OK;
	if((rc = item_fill(ctx, S, d_ol, n_ol, B, n_items)) != PCR_OK) return rc;
	const uint32_t ni = (uint32_t)n_items;
	const unsigned grid_i = (ni + POOL_THREADS - 1)/POOL_THREADS;
	if((rc = X.cnt.ensure((size_t)ni + 1)) != PCR_OK) return rc;                // (the entry counts are spent)
	// ---- with a rule: the 3' end per item
	const ItemEnd *d_item_end = nullptr;
	if(ruled && (rc = end3_items(ctx, S, ni, d_ol, d_norm, R.window, use_taq, d_item_end)) != PCR_OK) return rc;
	// ---- 2. job offsets, the jobs; 3. Tm per item
	if((rc = melt_items(who, ctx, S, d_ol, d_olx, ni, args->salt, B)) != PCR_OK) return rc;
	// ---- 4. the join: count, scan, emit
	const uint32_t seq_bits = pool_bits(S.n);
	const JoinIn J{S.db.p, S.db_cap, S.touched.p, S.d_seg_hi, X.items.p, ni, X.eoff.p, d_ol, n_ol, S.planes.p, S.d_blk_off.p, S.d_len.p,
		S.d_has_eos.p, amp_min, amp_max};
	hipLaunchKernelGGL(k_conflict_join<false>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, (const ItemTm *)X.item_tm.p, tm_floor, d_item_end, R, d_intended,
		d_rows_off, d_rows, d_row_ol, n_pool, seq_bits, X.cnt.p, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr);
	HIP_TRY(hipGetLastError());
	uint64_t total = 0;
	uint32_t bad = 0;
	if((rc = scan_total(ctx, X.cnt.p, ctx->pcf_aoff, X.tmp, ni, total, [&]() -> int {
		HIP_TRY(hipMemcpyAsync(&bad, X.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		return PCR_OK;
	})) != PCR_OK) return rc;
	if(bad & 1u){ g_err = who + ": internal trace-back error"; return PCR_ERR_RANGE; }
	if(total >= PCF_MAX_ATTRIBUTIONS){ g_err = who + ": 2^31 or more (product, cell) attributions"; return PCR_ERR_CAPACITY; }
	if(total == 0) return PCR_OK;
	const uint32_t na = (uint32_t)total;
	if((rc = ctx->pcf_keys.ensure(2*(size_t)na)) != PCR_OK) return rc;
	if((rc = ctx->pcf_vals.ensure(2*(size_t)na)) != PCR_OK) return rc;
	uint64_t *k0 = ctx->pcf_keys.p, *k1 = k0 + na;
	uint32_t *v0 = ctx->pcf_vals.p, *v1 = v0 + na;
	hipLaunchKernelGGL(k_conflict_join<true>, dim3(grid_i), dim3(POOL_THREADS), 0, ctx->stream, J, (const ItemTm *)X.item_tm.p, tm_floor, d_item_end, R, d_intended,
		d_rows_off, d_rows, d_row_ol, n_pool, seq_bits, (uint32_t *)nullptr, (const uint64_t *)ctx->pcf_aoff.p, k0, v0);
	HIP_TRY(hipGetLastError());
	// ---- 5. (cell, sequence) order, then one aggregate per cell
	const uint32_t n_slots = std::min(na, n_cells);                              // the cells with a product
	if((rc = ctx->pcf_ucell.ensure((size_t)n_slots + 1)) != PCR_OK) return rc;   // (+ the count)
	if((rc = ctx->pcf_uagg.ensure(n_slots)) != PCR_OK) return rc;
	uint32_t *d_n_unique = ctx->pcf_ucell.p + n_slots;
	const auto cells_in = rocprim::make_transform_iterator((const uint64_t *)k1, PcfCellOf{seq_bits});
	PcfAggOf agg_of; agg_of.key = k1; agg_of.val = v1; agg_of.seq_mask = (1ull << seq_bits) - 1ull;
	const auto aggs_in = rocprim::make_transform_iterator(rocprim::make_counting_iterator(uint32_t(0)), agg_of);
	size_t t1 = 0, t2 = 0;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, k0, k1, v0, v1, na, 0, seq_bits + PCF_CELL_BITS, ctx->stream));
	HIP_TRY(rocprim::reduce_by_key(nullptr, t2, cells_in, aggs_in, na, ctx->pcf_ucell.p, (ConflictAgg *)ctx->pcf_uagg.p, d_n_unique,
		PcfMerge(), rocprim::equal_to<uint32_t>(), ctx->stream));
	if((rc = ctx->shared.tmp.ensure(std::max(t1, t2) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->shared.tmp.p, t1, k0, k1, v0, v1, na, 0, seq_bits + PCF_CELL_BITS, ctx->stream));
	HIP_TRY(rocprim::reduce_by_key(ctx->shared.tmp.p, t2, cells_in, aggs_in, na, ctx->pcf_ucell.p, (ConflictAgg *)ctx->pcf_uagg.p, d_n_unique,
		PcfMerge(), rocprim::equal_to<uint32_t>(), ctx->stream));
	// ---- 6. into the dense array
	const unsigned grid_u = std::max(1u, std::min<unsigned>((n_slots + POOL_THREADS - 1)/POOL_THREADS, ctx->n_cu*8));
	hipLaunchKernelGGL(k_conflict_scatter, dim3(grid_u), dim3(POOL_THREADS), 0, ctx->stream, (const uint32_t *)ctx->pcf_ucell.p,
		(const ConflictAgg *)ctx->pcf_uagg.p, (const uint32_t *)d_n_unique, n_cells, (ConflictAgg *)ctx->pcf_dense.p);
	HIP_TRY(hipGetLastError());
	return PCR_OK;
}

// Step 7: tm_max of every ordered cell of pcr_pool_dimers' matrix (tm_floor = 0) in ctx->pcf_dmat[n_ol*n_ol].  The plan is
// pcr_pool_dimers', restated: the kernels read it as that call uploads it.
int conflict_dimers(const std::string &who, pcr_ctx *ctx, const pcr_thermo_args *args, const std::vector<DimerOligo> &ol, const std::vector<uint32_t> &pref, const std::vector<uint32_t> &row, const std::vector<float> &logs, uint32_t n_cls)
{
	int rc;
	const uint32_t n = (uint32_t)ol.size();
	const uint64_t n_cells = (uint64_t)n*n;
	const size_t ol_bytes = (size_t)n*sizeof(DimerOligo), pre_bytes = (size_t)(n + 1)*sizeof(uint32_t), log_bytes = logs.size()*sizeof(float);
	std::vector<uint8_t> blob(ol_bytes + 2*pre_bytes + log_bytes);
	memcpy(blob.data(), ol.data(), ol_bytes);
	memcpy(blob.data() + ol_bytes, pref.data(), pre_bytes);
	memcpy(blob.data() + ol_bytes + pre_bytes, row.data(), pre_bytes);
	memcpy(blob.data() + ol_bytes + 2*pre_bytes, logs.data(), log_bytes);
	if((rc = ctx->pcf_din.ensure(blob.size())) != PCR_OK) return rc;
	HIP_TRY(hipMemcpyAsync(ctx->pcf_din.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));                                   // (blob is this function's)
	DimerPlan P;
	P.ol = (const DimerOligo *)ctx->pcf_din.p;
	P.pref = (const uint32_t *)(ctx->pcf_din.p + ol_bytes);
	P.row = (const uint32_t *)(ctx->pcf_din.p + ol_bytes + pre_bytes);
	P.log_off = (const float *)(ctx->pcf_din.p + ol_bytes + 2*pre_bytes);
	P.log_diag = P.log_off + (size_t)n_cls*n_cls;
	P.n = n; P.n_cls = n_cls;
	if((rc = ensure_dg_table(ctx, args->salt)) != PCR_OK) return rc;
	if(!ctx->pdim_attr_set){                                                   // (k_pool_dimer's own flag: the attribute is the kernel's)
		HIP_TRY(hipFuncSetAttribute((const void *)k_pool_dimer, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PDIM_LDS));
		ctx->pdim_attr_set = true;
	}
	if((rc = ctx->pcf_dmat.ensure(n_cells)) != PCR_OK) return rc;
	auto before = [&](uint64_t c) -> uint32_t {
		if(c >= n_cells) return row[n];
		const uint32_t q = (uint32_t)(c/n), t = (uint32_t)(c % n);
		return pdim_before(row.data(), pref.data(), q, t, ol[q].n_exp);
	};
	const float log_na = logf(args->salt);
	uint64_t c0 = 0;
	while(c0 < n_cells){
		// ---- a batch: cells c0 .. c1 - 1; it closes before the cell that would take it past POOL_DIMER_BATCH_JOBS duplexes
		const uint32_t j0 = before(c0);
		uint64_t c1 = c0 + 1, above = n_cells + 1;
		while(above - c1 > 1){
			const uint64_t mid = c1 + (above - c1)/2;
			if(before(mid) - j0 <= POOL_DIMER_BATCH_JOBS) c1 = mid; else above = mid;
		}
		const uint32_t n_jobs = before(c1) - j0, nc = (uint32_t)(c1 - c0);
		if((rc = ctx->pcf_dres.ensure(n_jobs)) != PCR_OK) return rc;
		if((rc = ctx->pcf_drec.ensure(nc)) != PCR_OK) return rc;
		if((rc = ctx->pcf_dkeep.ensure((size_t)nc + 1)) != PCR_OK) return rc;
		const unsigned grid_j = std::max(1u, std::min<unsigned>((n_jobs + PDIM_WAVES - 1)/PDIM_WAVES, (unsigned)ctx->n_cu));
		hipLaunchKernelGGL(k_pool_dimer, dim3(grid_j), dim3(PDIM_THREADS), PDIM_LDS, ctx->stream, P, j0, n_jobs, (const int *)ctx->th_dg.p, log_na, ctx->pcf_dres.p);
		HIP_TRY(hipGetLastError());
		const unsigned grid_c = (nc + POOL_THREADS - 1)/POOL_THREADS;
		hipLaunchKernelGGL(k_pool_dimer_reduce, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, P, (uint32_t)c0, nc, j0, (const float4 *)ctx->pcf_dres.p,
			0.0f, ctx->pcf_drec.p, ctx->pcf_dkeep.p, ctx->shared.flag.p + 1);
		HIP_TRY(hipGetLastError());
		hipLaunchKernelGGL(k_conflict_dimer_store, dim3(grid_c), dim3(POOL_THREADS), 0, ctx->stream, (const pcr_pool_dimer *)ctx->pcf_drec.p, nc, ctx->pcf_dmat.p + c0);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipStreamSynchronize(ctx->stream));                                 // the next batch reuses the scratch
		c0 = c1;
	}
	uint32_t bad = 0;
	HIP_TRY(hipMemcpyAsync(&bad, ctx->shared.flag.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(bad & 1u){ g_err = who + ": internal trace-back error"; return PCR_ERR_RANGE; }
	return PCR_OK;
}

// What pcr_pool_dimers asks of primer_strand under `rule`, and its log strand concentrations: the degeneracy class of every oligo
// (q.cls, cls_degen) and logs[n_cls*n_cls + n_cls] as pdim_host_plan lays them out.  what: the argument that asked, for the refusals.
int conflict_dimer_logs(const std::string &who, const char *what, const pcr_thermo_args *args, int rule, std::vector<DimerOligo> &dol,
	std::vector<uint32_t> &cls_degen, std::vector<float> &logs)
{
	if(!(args->primer_strand > 0.0f)){ g_err = who + ": with " + what + " primer_strand must be positive (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	cls_degen.clear();
	for(DimerOligo &q : dol){
		const auto at = std::find(cls_degen.begin(), cls_degen.end(), q.n_exp);
		q.cls = (uint32_t)(at - cls_degen.begin());
		if(at == cls_degen.end()) cls_degen.push_back(q.n_exp);
	}
	const uint32_t n_cls = (uint32_t)cls_degen.size();
	logs.assign((size_t)n_cls*n_cls + n_cls, 0.0f);
	for(uint32_t a = 0;a < n_cls;++a){
		const float ca = (float)(args->primer_strand/(double)cls_degen[a]);
		for(uint32_t b = 0;b < n_cls;++b){
			const float cb = (float)(args->primer_strand/(double)cls_degen[b]);
			const float strand = (rule == PCR_DIMER_RULE_POOL) ? args->primer_strand                      // pcr_assay.cpp:819-821
				: ((ca > cb) ? ca - 0.5f*cb : cb - 0.5f*ca);                                            // pcr_assay.cpp:244, nuc_cruc.h:832-837
			if(!(strand > 0.0f)){ g_err = who + ": primer_strand / degeneracy underflows to zero"; return PCR_ERR_ARG; }
			logs[(size_t)a*n_cls + b] = logf(strand);
		}
		const float own = (rule == PCR_DIMER_RULE_POOL) ? args->primer_strand : ca;                       // valid_pcr.cpp:13
		if(!(own > 0.0f)){ g_err = who + ": primer_strand / degeneracy underflows to zero"; return PCR_ERR_ARG; }
		logs[(size_t)n_cls*n_cls + a] = logf(own);
	}
	return PCR_OK;
}

// pcr_pool_conflicts_ext's side of pool_conflicts_impl (pcr_pool_conflicts_ext.inc): its arguments, and the tail that joins the
// extension half to the cells' records (pcf_rec, pcf_keep) and hands out the 96-byte records.
struct ConflictExt { const pcr_dimer_end3_args *ext; pcr_pool_conflict_ext *out; };
int conflict_ext_check(const std::string &who, const pcr_dimer_end3_args *ext);
int64_t conflict_ext_tail(const std::string &who, pcr_ctx *ctx, const pcr_thermo_args *args, const ConflictExt &X, const DimerHostPlan *H,
	const uint2 *d_row_ol, uint32_t n_pool, uint32_t n_cells, uint64_t cap);

// pcr_pool_conflicts (rule = NULL), pcr_pool_conflicts_end3 and, with X, pcr_pool_conflicts_ext (out = NULL then: the records go
// to X->out); who: the entry point's name, for the refusals
int64_t pool_conflicts_impl(const std::string &who, pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor, const pcr_end3_rule *rule,
	int dimer_rule, float dimer_floor, uint32_t *oligo_id, pcr_pool_conflict *out, uint64_t cap, const ConflictExt *X = nullptr)
{
	static_assert(sizeof(pcr_pool_conflict) == 48, "record layout");
	static_assert(sizeof(ConflictAgg) == 16 && sizeof(uint4) == 16, "the dense array is kept as uint4");
	// ---- the arguments, before the handle (pcr_pool_products_tm's checks in its order, the oligo table, then the dimer arguments)
	if(!set_ok(which)){ g_err = who + ": unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = who + ": PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if(!args || (n_pool && (!pool || !oligo_id)) || (cap && !(X ? (const void *)X->out : (const void *)out))){ g_err = who + ": bad argument"; return PCR_ERR_ARG; }
	if(n_pool > PCR_POOL_MAX_PAIRS){ g_err = who + ": pool larger than PCR_POOL_MAX_PAIRS"; return PCR_ERR_ARG; }
	if(!(template_strand >= 0.0f) || !(args->primer_strand >= 0.0f)){ g_err = who + ": negative strand concentration (NucCruc::strand, nuc_cruc.h:818-826)"; return PCR_ERR_ARG; }
	if(!(args->salt >= 1.0e-6f && args->salt <= 1.0f)){ g_err = who + ": salt outside [1e-6, 1] (NucCruc::salt, nuc_cruc.h:780-788)"; return PCR_ERR_ARG; }
	std::vector<PoolOligo> ol;
	std::vector<SiteOligoX> olx;
	if(site_oligo_table(who, "an oligo", "primer_strand", pool, n_pool, threshold, args, template_strand, oligo_id, ol, olx) != PCR_OK) return PCR_ERR_ARG;
	std::vector<DimerOligo> dol;                                                 // pcr_pool_dimers' records of the same oligos
	for(uint32_t s = 0;s < 2*n_pool;++s){
		if(oligo_id[s] != dol.size()) continue;                                  // (ids count up in order of first appearance)
		DimerOligo q;
		q.m = pcrhost::planes_of_word(((s & 1) ? pool[s/2].r : pool[s/2].f).w);
		q.start = pcrhost::planes_start(q.m); q.stop = pcrhost::planes_stop(q.m);
		q.n_exp = olx[dol.size()].n_exp; q.cls = 0;
		dol.push_back(q);
	}
	if(!std::isfinite(tm_floor)){ g_err = who + ": tm_floor is not finite"; return PCR_ERR_ARG; }
	if(dimer_rule != PCR_DIMER_RULE_POOL && dimer_rule != PCR_DIMER_RULE_ASSAY && dimer_rule != PCR_CONFLICT_NO_DIMERS){
		g_err = who + ": unknown dimer_rule (PCR_DIMER_RULE_POOL, PCR_DIMER_RULE_ASSAY or PCR_CONFLICT_NO_DIMERS)"; return PCR_ERR_ARG;
	}
	if(!std::isfinite(dimer_floor)){ g_err = who + ": dimer_floor is not finite"; return PCR_ERR_ARG; }
	const bool dimers = dimer_rule != PCR_CONFLICT_NO_DIMERS;
	// with a dimer rule, what pcr_pool_dimers asks of the arguments: its strand concentrations, per pair of degeneracy classes
	std::vector<uint32_t> cls_degen, pref, row;
	std::vector<float> logs;
	if(dimers && conflict_dimer_logs(who, "a dimer rule", args, dimer_rule, dol, cls_degen, logs) != PCR_OK) return PCR_ERR_ARG;
	End3Rule R;
	int use_taq;
	if(end3_rule_of(who, rule, R, use_taq) != PCR_OK) return PCR_ERR_ARG;
	const bool ruled = end3_ruled(R);                                            // else: no ItemEnd is computed, the join is the base call's
	// with ext, what pcr_pool_dimers_end3 asks of its arguments, and its plan of the same oligos under ext->rule
	const bool extend = X && X->ext;
	DimerHostPlan XH;
	if(extend){
		if(conflict_ext_check(who, X->ext) != PCR_OK) return PCR_ERR_ARG;
		std::vector<uint32_t> xcls;
		if(conflict_dimer_logs(who, "ext", args, X->ext->rule, dol, xcls, XH.logs) != PCR_OK) return PCR_ERR_ARG;   // (the classes are the same under every rule)
		XH.n_cls = (uint32_t)xcls.size();
	}
	if(!ctx){ g_err = who + ": null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(!S.have_db){ g_err = who + ": no word DB (call pcr_select_words or pcr_select_sites first)"; return PCR_ERR_STATE; }
	if(n_pool == 0) return 0;
	const uint32_t n_ol = (uint32_t)ol.size();
	if(dimers || extend){
		// pcr_pool_dimers' duplex numbering: pref[t] = expansions of the oligos before t; row[q] = duplexes of the rows before q
		pref.assign(n_ol + 1, 0); row.assign(n_ol + 1, 0);
		for(uint32_t t = 0;t < n_ol;++t) pref[t + 1] = pref[t] + dol[t].n_exp;
		uint64_t total = 0;
		for(uint32_t q = 0;q < n_ol;++q){
			row[q] = (uint32_t)total;
			total += (uint64_t)dol[q].n_exp*(pref[n_ol] - dol[q].n_exp) + dol[q].n_exp;
			if(total >= (uint64_t(1) << 31)){ g_err = who + ": the pool's duplexes number 2^31 or more"; return PCR_ERR_CAPACITY; }
		}
		row[n_ol] = (uint32_t)total;
	}
	if(extend){ XH.ol = dol; XH.pref = pref; XH.row = row; XH.n = n_ol; }
	{ const int erc = ensure_touched(ctx, S); if(erc != PCR_OK) return erc; }
	int rc;
	const uint32_t n_cells = n_pool*(n_pool + 1u)/2u;
	if((rc = ctx->shared.flag.ensure(2)) != PCR_OK) return rc;                      // [0]: k_item_tm's (melt_items zeroes it), [1]: k_pool_dimer_reduce's
	HIP_TRY(hipMemsetAsync(ctx->shared.flag.p + 1, 0, sizeof(uint32_t), ctx->stream));
	if((rc = ctx->pcf_dense.ensure(n_cells)) != PCR_OK) return rc;
	HIP_TRY(hipMemsetAsync(ctx->pcf_dense.p, 0, (size_t)n_cells*sizeof(uint4), ctx->stream));
	if((rc = conflict_products(who, ctx, S, ol, olx, oligo_id, n_pool, amp_min, amp_max, args, tm_floor, R, ruled, use_taq, n_cells)) != PCR_OK) return rc;
	if(dimers && (rc = conflict_dimers(who, ctx, args, dol, pref, row, logs, (uint32_t)cls_degen.size())) != PCR_OK) return rc;
	// ---- 8. the records, the kept ones in (row_a, row_b) order
	const size_t ol_bytes = ol.size()*sizeof(PoolOligo), olx_bytes = olx.size()*sizeof(SiteOligoX);
	const uint2 *d_row_ol = (const uint2 *)(ctx->shared.in.p + ol_bytes + olx_bytes);   // (conflict_products' upload)
	if((rc = ctx->pcf_rec.ensure(n_cells)) != PCR_OK) return rc;
	if((rc = ctx->pcf_keep.ensure((size_t)n_cells + 1)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_conflict_cells, dim3((n_pool + POOL_THREADS - 1)/POOL_THREADS, n_pool), dim3(POOL_THREADS), 0, ctx->stream,
		(const ConflictAgg *)ctx->pcf_dense.p, dimers ? (const float *)ctx->pcf_dmat.p : (const float *)nullptr, n_ol, d_row_ol, n_pool, dimer_floor,
		ctx->pcf_rec.p, ctx->pcf_keep.p);
	HIP_TRY(hipGetLastError());
	if(X) return conflict_ext_tail(who, ctx, args, *X, extend ? &XH : nullptr, d_row_ol, n_pool, n_cells, cap);
	uint32_t kept = 0;
	if((rc = scan_total(ctx, ctx->pcf_keep.p, ctx->pcf_koff, ctx->shared.tmp, n_cells, kept)) != PCR_OK) return rc;
	if(kept == 0 || kept > cap) return (int64_t)kept;                            // count only: out is left as it is
	if((rc = ctx->pcf_out.ensure(kept)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_conflict_compact, dim3((n_cells + POOL_THREADS - 1)/POOL_THREADS), dim3(POOL_THREADS), 0, ctx->stream,
		(const pcr_pool_conflict *)ctx->pcf_rec.p, (const uint32_t *)ctx->pcf_keep.p, (const uint32_t *)ctx->pcf_koff.p, n_cells, ctx->pcf_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(out, ctx->pcf_out.p, (size_t)kept*sizeof(pcr_pool_conflict), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)kept;
}

} // namespace

extern "C" {

int64_t pcr_pool_conflicts(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	int dimer_rule, float dimer_floor, uint32_t *oligo_id, pcr_pool_conflict *out, uint64_t cap)
{
	return pool_conflicts_impl("pcr_pool_conflicts", ctx, which, pool, n_pool, threshold, amp_min, amp_max, args, template_strand, tm_floor, nullptr,
		dimer_rule, dimer_floor, oligo_id, out, cap);
}

int64_t pcr_pool_conflicts_end3(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, int dimer_rule, float dimer_floor, uint32_t *oligo_id, pcr_pool_conflict *out, uint64_t cap)
{
	return pool_conflicts_impl("pcr_pool_conflicts_end3", ctx, which, pool, n_pool, threshold, amp_min, amp_max, args, template_strand, tm_floor, rule,
		dimer_rule, dimer_floor, oligo_id, out, cap);
}

} // extern "C"

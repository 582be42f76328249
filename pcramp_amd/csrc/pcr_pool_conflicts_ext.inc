// pcr_pool_conflicts with the 3'-extensible dimers of pcr_pool_dimers_end3 folded in (pcr_pool_conflicts_ext; included by
// pcr_device.hip after pcr_pool_conflicts.inc, whose pool_conflicts_impl runs the argument checks and steps 1-8 and then calls
// conflict_ext_tail here, and after pcr_pool_dimers_end3.inc, whose batch loop it runs).
//   9.  With ext: end3_batches with a dense target.  Every batch merges its cell records in place at [c0, c1) of
//       pcr_ctx::pcx_dense, n_ol x n_ol records of 48 bytes (cell q*n_ol + t); nothing is compacted or downloaded.
//   10. k_conflict_ext_cells: a thread per cell a <= b reads the record and keep word step 8 left, sorts the (up to eight) ordered
//       dimer cells, skips the repeats, sums n_placements, counts the cells the dG filter keeps and takes the best of them:
//       lowest dG, then the longer run, then (walking in ascending order) the lowest (q, t).  Plain loads and compares in a fixed
//       order, no atomics: two runs give the same bytes.  scan_total and k_conflict_ext_compact put the kept 96-byte records
//       into (row_a, row_b) order.
// With ext = NULL step 9 is skipped and step 10 only widens the records.

namespace {

// Cell {a, b}, a = blockIdx.y <= b: base[c] and keep[c] are k_conflict_cells'; keep[c] becomes the ext call's keep word.
// dense = NULL: no extension half was asked for.
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_ext_cells(const pcr_pool_conflict *__restrict__ base, const pcr_pool_dimer_end3 *__restrict__ dense,
	uint32_t n_ol, const uint2 *__restrict__ row_ol, uint32_t n_pool, int keep_all, float dg_max, pcr_pool_conflict_ext *__restrict__ rec, uint32_t *keep)
{
	const uint32_t a = blockIdx.y, b = blockIdx.x*blockDim.x + threadIdx.x;
	if(b >= n_pool || b < a) return;
	const uint32_t c = pcf_cell(a, b, n_pool);
	pcr_pool_conflict_ext r;
	r.c = base[c];
	r.ext_cells = r.ext_placements = 0u;
	r.ext_query = r.ext_target = r.ext_q_expansion = r.ext_t_expansion = 0u;
	r.ext_run = r.ext_extension = r.ext_overlap = r.ext_overlap_matches = 0;
	r.ext_flags = 0u;
	r.ext_dG = r.ext_tm = r.ext_dH = r.ext_dS = 0.0f;
	if(dense){
		const uint2 oa = row_ol[a], ob = row_ol[b];
		// the (up to eight) ordered cells as q*n_ol + t, ascending: repeats are neighbours, and the first of the best is the lowest (q, t)
		uint32_t cell[8] = {oa.x*n_ol + ob.x, oa.x*n_ol + ob.y, oa.y*n_ol + ob.x, oa.y*n_ol + ob.y,
			ob.x*n_ol + oa.x, ob.y*n_ol + oa.x, ob.x*n_ol + oa.y, ob.y*n_ol + oa.y};
		for(int i = 1;i < 8;++i){
			for(int j = i;j > 0 && cell[j - 1] > cell[j];--j){ const uint32_t s = cell[j]; cell[j] = cell[j - 1]; cell[j - 1] = s; }
		}
		pcr_pool_dimer_end3 best = dense[cell[0]];
		for(int i = 0;i < 8;++i){
			if(i > 0 && cell[i] == cell[i - 1]) continue;
			const pcr_pool_dimer_end3 d = dense[cell[i]];
			r.ext_placements += d.n_placements;
			if(!(d.n_placements > 0u && (keep_all || d.dG <= dg_max))) continue;      // k_dimer_end3_cell_keep's test
			if(r.ext_cells == 0u || d.dG < best.dG || (d.dG == best.dG && d.run > best.run)) best = d;
			++r.ext_cells;
		}
		if(r.ext_cells){
			r.ext_query = best.query_oligo; r.ext_target = best.target_oligo;
			r.ext_q_expansion = best.q_expansion; r.ext_t_expansion = best.t_expansion;
			r.ext_run = best.run; r.ext_extension = best.extension; r.ext_overlap = best.overlap; r.ext_overlap_matches = best.overlap_matches;
			r.ext_flags = best.flags;
			r.ext_dG = best.dG; r.ext_tm = best.tm; r.ext_dH = best.dH; r.ext_dS = best.dS;
			r.c.flags |= PCR_CONFLICT_EXTENSION;
		}
	}
	rec[c] = r;
	keep[c] = (keep[c] || r.ext_cells) ? 1u : 0u;
}

// the kept cells, in cell order: off = exclusive scan of keep
__global__ __launch_bounds__(POOL_THREADS) void k_conflict_ext_compact(const pcr_pool_conflict_ext *__restrict__ rec, const uint32_t *__restrict__ keep,
	const uint32_t *__restrict__ off, uint32_t n_cells, pcr_pool_conflict_ext *__restrict__ out)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k < n_cells && keep[k]) out[off[k]] = rec[k];
}

// what pcr_pool_dimers_end3 asks of the arguments that ext carries, in its order
int conflict_ext_check(const std::string &who, const pcr_dimer_end3_args *ext)
{
	if(ext->rule != PCR_DIMER_RULE_POOL && ext->rule != PCR_DIMER_RULE_ASSAY){ g_err = who + ": unknown ext->rule (PCR_DIMER_RULE_POOL or PCR_DIMER_RULE_ASSAY)"; return PCR_ERR_ARG; }
	if(ext->min_run < 3u || ext->min_run > 32u){ g_err = who + ": ext->min_run outside 3 .. 32 (the engine gives no energy to a duplex of 1 or 2 bases)"; return PCR_ERR_ARG; }
	if(ext->min_extension > 31u){ g_err = who + ": ext->min_extension above 31"; return PCR_ERR_ARG; }
	if(ext->dg_max != ext->dg_max){ g_err = who + ": ext->dg_max is not a number"; return PCR_ERR_ARG; }
	return PCR_OK;
}

// Steps 9 and 10, after k_conflict_cells: H = the plan of the pool's oligos under ext->rule, NULL without ext.
int64_t conflict_ext_tail(const std::string &who, pcr_ctx *ctx, const pcr_thermo_args *args, const ConflictExt &X, const DimerHostPlan *H,
	const uint2 *d_row_ol, uint32_t n_pool, uint32_t n_cells, uint64_t cap)
{
	static_assert(sizeof(pcr_pool_conflict_ext) == 96 && sizeof(pcr_dimer_end3_args) == 16, "record layout");
	int rc;
	const pcr_pool_dimer_end3 *dense = nullptr;
	uint32_t n_ol = 0;
	float dg_max = INFINITY;
	if(H){
		n_ol = H->n; dg_max = X.ext->dg_max;
		if((rc = ctx->pcx_dense.ensure((size_t)n_ol*n_ol)) != PCR_OK) return rc;
		End3Out O;
		O.dense = ctx->pcx_dense.p;
		uint64_t kept_cells = 0, kept_places = 0;
		if((rc = end3_batches(who.c_str(), ctx, *H, args, X.ext->min_run, X.ext->min_extension, dg_max, O, kept_cells, kept_places)) != PCR_OK) return rc;
		dense = ctx->pcx_dense.p;
	}
	if((rc = ctx->pcx_rec.ensure(n_cells)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_conflict_ext_cells, dim3((n_pool + POOL_THREADS - 1)/POOL_THREADS, n_pool), dim3(POOL_THREADS), 0, ctx->stream,
		(const pcr_pool_conflict *)ctx->pcf_rec.p, dense, n_ol, d_row_ol, n_pool, (dg_max == INFINITY) ? 1 : 0, dg_max, ctx->pcx_rec.p, ctx->pcf_keep.p);
	HIP_TRY(hipGetLastError());
	uint32_t kept = 0;
	if((rc = scan_total(ctx, ctx->pcf_keep.p, ctx->pcf_koff, ctx->shared.tmp, n_cells, kept)) != PCR_OK) return rc;
	if(kept == 0 || kept > cap) return (int64_t)kept;                            // count only: out is left as it is
	if((rc = ctx->pcx_out.ensure(kept)) != PCR_OK) return rc;
	hipLaunchKernelGGL(k_conflict_ext_compact, dim3((n_cells + POOL_THREADS - 1)/POOL_THREADS), dim3(POOL_THREADS), 0, ctx->stream,
		(const pcr_pool_conflict_ext *)ctx->pcx_rec.p, (const uint32_t *)ctx->pcf_keep.p, (const uint32_t *)ctx->pcf_koff.p, n_cells, ctx->pcx_out.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(X.out, ctx->pcx_out.p, (size_t)kept*sizeof(pcr_pool_conflict_ext), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)kept;
}

} // namespace

extern "C" {

int64_t pcr_pool_conflicts_ext(pcr_ctx *ctx, pcr_set which, const pcr_pair *pool, uint32_t n_pool, float threshold,
	int32_t amp_min, int32_t amp_max, const pcr_thermo_args *args, float template_strand, float tm_floor,
	const pcr_end3_rule *rule, int dimer_rule, float dimer_floor, const pcr_dimer_end3_args *ext,
	uint32_t *oligo_id, pcr_pool_conflict_ext *out, uint64_t cap)
{
	const ConflictExt X{ext, out};
	return pool_conflicts_impl("pcr_pool_conflicts_ext", ctx, which, pool, n_pool, threshold, amp_min, amp_max, args, template_strand, tm_floor, rule,
		dimer_rule, dimer_floor, oligo_id, nullptr, cap, &X);
}

} // extern "C"

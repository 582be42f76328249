// The bases of a set of products: length, G+C, which records spell the same amplicon, and the unique amplicons packed
// (pcr_pool_amplicons; included by pcr_device.hip after pcr_probe_hits.inc).
//
// The host turns each record into an interval {sequence, start, length} of the loaded set, checked against the set's lengths:
// no kernel is handed an interval it has not seen pass.  From there:
//   1. k_amp_scan: one group of 8 lanes per record (8 records per wave), lane l of the group takes the 32-base blocks l, l + 8, ...
//      of the region.  A block is two uint4 plane loads funnel-shifted to the region's start (the second is the next block or the
//      sequence's zero halo); the reverse complement's block j is the mirrored forward window bit-reversed with the planes
//      exchanged (A <-> T, C <-> G).  gc and other are popcounts over the planes.  Each block gives a 64-bit hash mixed with its
//      number, the group's sums are the hashes of the two spellings.  canonical: the first block (lowest pass, then lowest lane of
//      the group's bits of a ballot) in which the two spellings differ decides, at its lowest differing position, by the codes as
//      unsigned integers.
//   2. rocprim::radix_sort_pairs on the hash (mixed with the length) with the record index as value: stable, so a run of equal
//      keys lists its records by index and starts with the lowest.  k_amp_heads + a max-scan give every position its run's
//      start; k_amp_verify: one group per record compares its spelling with that of the run's first, block by block.  Equal:
//      the first is its representative.  Not equal (two spellings under one key): flagged.
//   3. Flagged records -- none unless a hash collides or PCRAMP_DEBUG_AMP_HASH_BITS narrows the key -- are spelled out by
//      k_amp_extract and grouped on the host by their bytes; equal spellings have equal keys, so a flagged record can only
//      equal other flagged records.  The classes never depend on the hash.
//   4. k_amp_count (copies by atomicAdd, the class heads, a (representative, sequence) key), an exclusive scan of the heads
//      (class ids by first appearance), radix_sort_keys + k_amp_seqs (distinct sequences per class), k_amp_info (the records,
//      and per class its first record, length and byte count), an exclusive scan of the byte counts.
//   5. k_amp_extract: one group per class, a lane per 32-base block = 16 whole bytes, so no two lanes share a byte.
// The call owns its scratch (pcr_ctx::pam_*).

namespace {

constexpr int AMP_WAVES = 4;                                                    // waves per block of the group-per-record kernels
constexpr uint32_t AMP_LANES = 8;                                               // lanes per record: products are 3 to 7 blocks of 32 bases, a whole wave per record would idle
constexpr uint32_t AMP_GROUPS = 64/AMP_LANES;                                   // records per wave
constexpr uint32_t AMP_BLOCK_RECORDS = AMP_WAVES*AMP_GROUPS;                    // records per workgroup
constexpr unsigned long long AMP_GROUP_MASK = (1ull << AMP_LANES) - 1ull;
constexpr uint32_t AMP_UNRESOLVED = 0xFFFFFFFFu;                                // rep[] of a flagged record

__device__ __forceinline__ uint64_t amp_mix(uint64_t x)
{
	x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
	return x;
}

// block j of a spelling as a hash: summed over the blocks (any order) it is position-weighted through j
__device__ __forceinline__ uint64_t amp_block_hash(const uint4 w, uint32_t j)
{
	const uint64_t v0 = ((uint64_t)w.y << 32) | w.x, v1 = ((uint64_t)w.w << 32) | w.z;
	return amp_mix(amp_mix(v0 + 0x9E3779B97F4A7C15ull*((uint64_t)j + 1ull)) ^ v1);
}

// the m <= 32 codes at pos .. pos + m - 1 of the sequence whose blocks start at `base`, as plane words (bit i = position pos + i);
// the bits from m on are clear.  pos < the sequence's length: block (pos >> 5) + 1 is a block of the sequence or its halo.
__device__ __forceinline__ uint4 amp_window(const uint4 *__restrict__ planes, uint64_t base, uint32_t pos, uint32_t m)
{
	const uint32_t b = pos >> 5, sh = pos & 31u;
	const uint4 lo = planes[base + b], hi = planes[base + b + 1];
	const uint32_t keep = (m >= 32u) ? 0xFFFFFFFFu : ((1u << m) - 1u);
	return make_uint4(funnel(lo.x, hi.x, sh) & keep, funnel(lo.y, hi.y, sh) & keep, funnel(lo.z, hi.z, sh) & keep, funnel(lo.w, hi.w, sh) & keep);
}

// block j (32*j < len) of the spelling of region [start, start + len): forward, or its reverse complement (words._COMP on planes:
// A <-> T, C <-> G)
__device__ __forceinline__ uint4 amp_block(const uint4 *__restrict__ planes, uint64_t base, uint32_t start, uint32_t len, uint32_t j, bool rev)
{
	const uint32_t left = len - 32u*j, m = (left < 32u) ? left : 32u;
	if(!rev) return amp_window(planes, base, start + 32u*j, m);
	const uint4 f = amp_window(planes, base, start + left - m, m);                // forward positions left - m .. left - 1: bit t -> bit m - 1 - t
	const uint32_t sh = 32u - m;
	return make_uint4(__brev(f.w) >> sh, __brev(f.z) >> sh, __brev(f.y) >> sh, __brev(f.x) >> sh);
}

__device__ __forceinline__ uint32_t amp_code(const uint4 w, uint32_t p)
{
	return ((w.x >> p) & 1u) | (((w.y >> p) & 1u) << 1) | (((w.z >> p) & 1u) << 2) | (((w.w >> p) & 1u) << 3);
}

// the sum over the AMP_LANES lanes of a group (xor steps below AMP_LANES stay inside the aligned group)
__device__ __forceinline__ uint64_t amp_group_sum(uint64_t v)
{
	for(int d = AMP_LANES/2;d >= 1;d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
	return v;
}

// One group of AMP_LANES lanes per record k = {sequence, start, length, -}, lane l of the group takes blocks l, l + AMP_LANES, ...:
// stat[k] = {gc, other, reversed, -}, key[k] = the hash of the chosen spelling mixed with the length (and narrowed by key_mask),
// ord[k] = k.  The groups of a wave loop together (as often as its longest record needs), so the ballots are the whole wave's and
// each group reads its own AMP_LANES bits of them.
__global__ __launch_bounds__(64*AMP_WAVES) void k_amp_scan(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint4 *__restrict__ iv, uint32_t n, int canonical, uint64_t key_mask, uint4 *__restrict__ stat, uint64_t *__restrict__ key,
	uint32_t *__restrict__ ord)
{
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	const uint32_t grp = lane/AMP_LANES, sub = lane % AMP_LANES, shift = grp*AMP_LANES;
	for(uint32_t k0 = (blockIdx.x*AMP_WAVES + wave)*AMP_GROUPS;k0 < n;k0 += gridDim.x*AMP_BLOCK_RECORDS){   // uniform per wave
		const uint32_t k = k0 + grp;
		const bool live = k < n;
		const uint4 r = live ? iv[k] : make_uint4(0u, 0u, 0u, 0u);
		const uint64_t base = live ? blk_off[r.x] : 0;
		const uint32_t start = r.y, len = r.z, nblk = (len + 31u) >> 5;            // (a group without a record has no block)
		uint32_t gc = 0, other = 0;
		uint64_t hf = 0, hr = 0;
		bool decided = false, rev = false;
		for(uint32_t j0 = 0;__any(j0 < nblk);j0 += AMP_LANES){                      // (uniform trip count: the ballots below are the whole wave's)
			const uint32_t j = j0 + sub;
			bool differ = false, less = false;
			if(j < nblk){
				const uint4 f = amp_block(planes, base, start, len, j, false);
				const uint32_t left = len - 32u*j, valid = (left >= 32u) ? 0xFFFFFFFFu : ((1u << left) - 1u);
				const uint32_t pairs = (f.x & f.y) | ((f.x | f.y) & (f.z | f.w)) | (f.z & f.w);   // two or more bases possible
				const uint32_t one = (f.x ^ f.y ^ f.z ^ f.w) & ~pairs;                            // exactly A, C, G or T
				gc += __popc(~f.x & ~f.w & (f.y | f.z));                                          // C, G or S
				other += __popc(valid & ~one);
				hf += amp_block_hash(f, j);
				if(canonical){
					const uint4 c = amp_block(planes, base, start, len, j, true);
					hr += amp_block_hash(c, j);
					const uint32_t d = (f.x ^ c.x) | (f.y ^ c.y) | (f.z ^ c.z) | (f.w ^ c.w);
					if(d){
						const uint32_t p = (uint32_t)__ffs((int)d) - 1u;
						differ = true; less = amp_code(c, p) < amp_code(f, p);
					}
				}
			}
			if(canonical){
				const unsigned long long dm = (__ballot(differ) >> shift) & AMP_GROUP_MASK, lm = (__ballot(less) >> shift) & AMP_GROUP_MASK;
				if(!decided && dm){ rev = ((lm >> (__ffsll((long long)dm) - 1)) & 1ull) != 0; decided = true; }
			}
		}
		gc = (uint32_t)amp_group_sum(gc); other = (uint32_t)amp_group_sum(other);
		hf = amp_group_sum(hf); hr = amp_group_sum(hr);
		if(live && sub == 0){
			stat[k] = make_uint4(gc, other, rev ? 1u : 0u, 0u);
			key[k] = amp_mix((rev ? hr : hf) + 0xD6E8FEB86659FD93ull*((uint64_t)len + 1ull)) & key_mask;
			ord[k] = k;
		}
	}
}

// sorted position r -> r if it starts a run of equal keys, else 0 (an inclusive max-scan then gives every position its run's start)
__global__ void k_amp_heads(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ head_pos)
{
	const uint32_t r = blockIdx.x*blockDim.x + threadIdx.x;
	if(r < n) head_pos[r] = (r > 0 && key[r] != key[r - 1]) ? r : 0u;
}

// One group of AMP_LANES lanes per sorted position r: record ord[r] against the first record of its run.  rep[record] = that first
// record, the record itself at a run's start, or AMP_UNRESOLVED (and *n_flag counts it) where the two spellings differ.
__global__ __launch_bounds__(64*AMP_WAVES) void k_amp_verify(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint4 *__restrict__ iv, const uint4 *__restrict__ stat, const uint32_t *__restrict__ ord, const uint32_t *__restrict__ run_start,
	uint32_t n, uint32_t *__restrict__ rep, uint32_t *__restrict__ n_flag)
{
	const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	const uint32_t grp = lane/AMP_LANES, sub = lane % AMP_LANES, shift = grp*AMP_LANES;
	for(uint32_t r0 = (blockIdx.x*AMP_WAVES + wave)*AMP_GROUPS;r0 < n;r0 += gridDim.x*AMP_BLOCK_RECORDS){   // uniform per wave
		const uint32_t r = r0 + grp;
		const bool live = r < n;
		const uint32_t g = live ? run_start[r] : 0u, k = live ? ord[r] : 0u;
		const bool head = live && g == r;
		const uint32_t f = (live && !head) ? ord[g] : k;
		uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
		if(live && !head){ a = iv[k]; b = iv[f]; }
		bool same = a.z == b.z;
		const bool compare = live && !head && same;
		const uint64_t base_a = compare ? blk_off[a.x] : 0, base_b = compare ? blk_off[b.x] : 0;
		const bool rev_a = compare && stat[k].z != 0, rev_b = compare && stat[f].z != 0;
		const uint32_t nblk = compare ? ((a.z + 31u) >> 5) : 0u;
		for(uint32_t j0 = 0;__any(j0 < nblk && same);j0 += AMP_LANES){               // (uniform trip count: the ballot below is the whole wave's)
			const uint32_t j = j0 + sub;
			bool differ = false;
			if(j < nblk && same){
				const uint4 x = amp_block(planes, base_a, a.y, a.z, j, rev_a), y = amp_block(planes, base_b, b.y, b.z, j, rev_b);
				differ = ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
			}
			if((__ballot(differ) >> shift) & AMP_GROUP_MASK) same = false;
		}
		if(live && sub == 0){
			rep[k] = head ? k : (same ? f : AMP_UNRESOLVED);
			if(!head && !same) atomicAdd(n_flag, 1u);
		}
	}
}

// per record: one more copy of its class, whether it heads the class, and the key of (class, sequence)
__global__ void k_amp_count(const uint4 *__restrict__ iv, const uint32_t *__restrict__ rep, uint32_t n, uint32_t *__restrict__ copies,
	uint32_t *__restrict__ head, uint64_t *__restrict__ seq_key)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n) return;
	const uint32_t r = rep[k];
	atomicAdd(copies + r, 1u);
	head[k] = (r == k) ? 1u : 0u;
	seq_key[k] = ((uint64_t)r << 32) | iv[k].x;
}

// the sorted (class, sequence) keys: every distinct one is one more sequence of its class
__global__ void k_amp_seqs(const uint64_t *__restrict__ seq_key, uint32_t n, uint32_t *__restrict__ n_seq)
{
	const uint32_t i = blockIdx.x*blockDim.x + threadIdx.x;
	if(i >= n) return;
	if(i == 0 || seq_key[i] != seq_key[i - 1]) atomicAdd(n_seq + (uint32_t)(seq_key[i] >> 32), 1u);
}

// info[k]; and for the head of class c: its record, length and byte count
__global__ void k_amp_info(const uint4 *__restrict__ iv, const uint4 *__restrict__ stat, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ cls,
	const uint32_t *__restrict__ copies, const uint32_t *__restrict__ n_seq, uint32_t n, pcr_amplicon_info *__restrict__ info,
	uint32_t *__restrict__ class_rec, uint64_t *__restrict__ class_len, uint32_t *__restrict__ class_bytes)
{
	const uint32_t k = blockIdx.x*blockDim.x + threadIdx.x;
	if(k >= n) return;
	const uint32_t r = rep[k], c = cls[r];
	const uint4 s = stat[k];
	pcr_amplicon_info o;
	o.length = iv[k].z; o.gc = s.x; o.other = s.y; o.flags = s.z ? PCR_AMPLICON_REVERSED : 0u;
	o.amplicon = c; o.first = r; o.copies = copies[r]; o.sequences = n_seq[r];
	info[k] = o;
	if(r == k){ class_rec[c] = k; class_len[c] = o.length; class_bytes[c] = (o.length + 1u) >> 1; }
}

// One group of AMP_LANES lanes per item c: the spelling of record item_rec[c], two codes per byte, high nibble first, an odd tail
// padded with 0, at out + item_off[c].  A lane writes the 16 bytes of a 32-base block (fewer in the last): whole bytes, no byte has
// two writers.
__global__ __launch_bounds__(64*AMP_WAVES) void k_amp_extract(const uint4 *__restrict__ planes, const uint64_t *__restrict__ blk_off,
	const uint4 *__restrict__ iv, const uint4 *__restrict__ stat, const uint32_t *__restrict__ item_rec, const uint64_t *__restrict__ item_off,
	uint32_t n_items, uint8_t *__restrict__ out)
{
	const uint32_t grp = threadIdx.x/AMP_LANES, sub = threadIdx.x % AMP_LANES;     // (no cross-lane step: the groups need not keep step)
	for(uint32_t c = blockIdx.x*AMP_BLOCK_RECORDS + grp;c < n_items;c += gridDim.x*AMP_BLOCK_RECORDS){
		const uint32_t k = item_rec[c];
		const uint4 r = iv[k];
		const uint64_t base = blk_off[r.x], off = item_off[c];
		const bool rev = stat[k].z != 0;
		const uint32_t nblk = (r.z + 31u) >> 5;
		for(uint32_t j = sub;j < nblk;j += AMP_LANES){
			const uint4 w = amp_block(planes, base, r.y, r.z, j, rev);
			uint32_t d[4] = {0, 0, 0, 0};                                             // byte t = codes 2t (high nibble), 2t + 1: byte t & 3 of d[t >> 2]
#pragma unroll
			for(uint32_t i = 0;i < 32;++i) d[i >> 3] |= amp_code(w, i) << (8u*((i >> 1) & 3u) + ((i & 1u) ? 0u : 4u));
			const uint32_t left = r.z - 32u*j, nbytes = (left >= 32u) ? 16u : ((left + 1u) >> 1);
			uint8_t *p = out + off + 16ull*j;
			if(nbytes == 16u && (off & 3ull) == 0){
				uint32_t *q = (uint32_t *)p;
				q[0] = d[0]; q[1] = d[1]; q[2] = d[2]; q[3] = d[3];
			}
			else for(uint32_t t = 0;t < nbytes;++t) p[t] = (uint8_t)(d[t >> 2] >> (8u*(t & 3u)));
		}
	}
}

// Record k's region as {sequence, start, length, 0} of the set S, checked against the set's lengths (an empty PCR_REGION_INSERT is
// {sequence, 0, 0, 0} wherever it lies): the one place a product record becomes an interval a kernel may read.  `who` names the
// entry point in the error text.
int product_interval(const char *who, const SeqSet &S, const pcr_product &p, uint32_t k, int region, uint4 &iv)
{
	if(p.sequence >= S.n){ g_err = std::string(who) + ": record " + std::to_string(k) + ": sequence " + std::to_string(p.sequence) + " is not in the set"; return PCR_ERR_ARG; }
	int64_t first, len;
	if(region == PCR_REGION_PRODUCT){ first = p.begin; len = (int64_t)p.end - p.begin + 1; }
	else if(region == PCR_REGION_INSERT){ first = (int64_t)p.inner_start + 4; len = (int64_t)p.inner_length - 12; }
	else{ first = p.inner_start; len = p.inner_length; }
	const bool empty_ok = region == PCR_REGION_INSERT && len == 0;
	if(!empty_ok && (len <= 0 || first < 0 || (uint64_t)(first + len) > S.len[p.sequence])){
		g_err = std::string(who) + ": record " + std::to_string(k) + ": region " + std::to_string(first) + " .. " + std::to_string(first + len - 1) +
			" lies outside sequence " + std::to_string(p.sequence) + " (" + std::to_string(S.len[p.sequence]) + " bases)";
		return PCR_ERR_ARG;
	}
	iv = make_uint4(p.sequence, empty_ok ? 0u : (uint32_t)first, (uint32_t)len, 0u);
	return PCR_OK;
}

} // namespace

extern "C" {

int64_t pcr_pool_amplicons(pcr_ctx *ctx, pcr_set which, const pcr_product *products, uint64_t n, int region, int canonical,
	pcr_amplicon_info *info, uint64_t *class_byte_offset, uint64_t *class_length, uint64_t class_cap,
	uint8_t *packed4, uint64_t packed_cap, uint64_t *packed_bytes)
{
	static_assert(sizeof(pcr_amplicon_info) == 32, "record layout");
	// ---- the arguments, before the handle
	if(!set_ok(which)){ g_err = "pcr_pool_amplicons: unknown sequence set"; return PCR_ERR_ARG; }
	if(which != PCR_SET_TARGET && which != PCR_SET_BACKGROUND){ g_err = "pcr_pool_amplicons: PCR_SET_MULTIPLEX is not supported (PCR_SET_TARGET or PCR_SET_BACKGROUND)"; return PCR_ERR_ARG; }
	if((n && !products) || (class_cap && (!class_byte_offset || !class_length)) || (packed_cap && !packed4)){ g_err = "pcr_pool_amplicons: bad argument"; return PCR_ERR_ARG; }
	if(region != PCR_REGION_PRODUCT && region != PCR_REGION_INSERT && region != PCR_REGION_INNER){ g_err = "pcr_pool_amplicons: unknown region (PCR_REGION_PRODUCT, PCR_REGION_INSERT or PCR_REGION_INNER)"; return PCR_ERR_ARG; }
	if(n >= (1ull << 31)){ g_err = "pcr_pool_amplicons: 2^31 or more records"; return PCR_ERR_ARG; }
	if(!ctx){ g_err = "pcr_pool_amplicons: null handle"; return PCR_ERR_ARG; }
	{ const int drc = drain(ctx); if(drc != PCR_OK) return drc; }
	HIP_TRY(hipSetDevice(ctx->device));
	SeqSet &S = ctx->sets[which];
	if(S.n == 0){ g_err = "pcr_pool_amplicons: the set is not loaded (call pcr_load_sequences first)"; return PCR_ERR_STATE; }
	if(packed_bytes) *packed_bytes = 0;
	if(n == 0) return 0;
	// ---- every record's interval, against the set's lengths: no kernel sees one that fails
	const uint32_t nr = (uint32_t)n;
	std::vector<uint4> iv(nr);
	for(uint32_t k = 0;k < nr;++k){
		const int irc = product_interval("pcr_pool_amplicons", S, products[k], k, region, iv[k]);
		if(irc != PCR_OK) return irc;
	}
	// ---- scratch: u32 and u64 arrays carved from one buffer each
	int rc;
	const size_t N = nr;
	if((rc = ctx->pam_iv.ensure(N)) != PCR_OK) return rc;
	if((rc = ctx->pam_stat.ensure(N)) != PCR_OK) return rc;
	if((rc = ctx->pam_u32.ensure(11*N + 4)) != PCR_OK) return rc;
	if((rc = ctx->pam_u64.ensure(4*N + 2)) != PCR_OK) return rc;
	if((rc = ctx->pam_info.ensure(N)) != PCR_OK) return rc;
	uint32_t *o0 = ctx->pam_u32.p, *o1 = o0 + N, *head_pos = o1 + N, *run_start = head_pos + N, *rep = run_start + N, *copies = rep + N,
		*n_seq = copies + N, *head = n_seq + N, *cls = head + N + 1, *class_rec = cls + N + 1, *class_bytes = class_rec + N, *n_flag = class_bytes + N + 1;
	uint64_t *k0 = ctx->pam_u64.p, *k1 = k0 + N, *class_off = k1 + N, *class_len = class_off + N + 1;
	HIP_TRY(hipMemcpyAsync(ctx->pam_iv.p, iv.data(), N*sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(hipMemsetAsync(copies, 0, 2*N*sizeof(uint32_t), ctx->stream));        // copies[] and n_seq[]
	HIP_TRY(hipMemsetAsync(n_flag, 0, sizeof(uint32_t), ctx->stream));
	// ---- 1. scan
	const unsigned grid_w = std::max(1u, std::min<unsigned>((nr + AMP_BLOCK_RECORDS - 1)/AMP_BLOCK_RECORDS, ctx->n_cu*16)), grid_t = (nr + 255)/256;
	const uint64_t key_mask = (ctx->amp_dbg_hash_bits && ctx->amp_dbg_hash_bits < 64) ? ((1ull << ctx->amp_dbg_hash_bits) - 1ull) : ~0ull;
	hipLaunchKernelGGL(k_amp_scan, dim3(grid_w), dim3(64*AMP_WAVES), 0, ctx->stream, (const uint4 *)S.planes.p, (const uint64_t *)S.d_blk_off.p,
		(const uint4 *)ctx->pam_iv.p, nr, canonical, key_mask, ctx->pam_stat.p, k0, o0);
	HIP_TRY(hipGetLastError());
	// ---- 2. runs of equal keys, every record against its run's first
	size_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
	const unsigned key_bits = (key_mask == ~0ull) ? 64u : ctx->amp_dbg_hash_bits;
	HIP_TRY(rocprim::radix_sort_pairs(nullptr, t0, k0, k1, o0, o1, nr, 0, key_bits, ctx->stream));
	HIP_TRY(rocprim::inclusive_scan(nullptr, t1, head_pos, run_start, N, rocprim::maximum<uint32_t>(), ctx->stream));
	HIP_TRY(rocprim::exclusive_scan(nullptr, t2, head, cls, uint32_t(0), N + 1, rocprim::plus<uint32_t>(), ctx->stream));
	HIP_TRY(rocprim::radix_sort_keys(nullptr, t3, k0, k1, nr, 0, 64, ctx->stream));
	HIP_TRY(rocprim::exclusive_scan(nullptr, t4, class_bytes, class_off, uint64_t(0), N + 1, rocprim::plus<uint64_t>(), ctx->stream));
	if((rc = ctx->pam_tmp.ensure(std::max(std::max(t0, t1), std::max(t2, std::max(t3, t4))) + 16)) != PCR_OK) return rc;
	HIP_TRY(rocprim::radix_sort_pairs(ctx->pam_tmp.p, t0, k0, k1, o0, o1, nr, 0, key_bits, ctx->stream));
	hipLaunchKernelGGL(k_amp_heads, dim3(grid_t), dim3(256), 0, ctx->stream, (const uint64_t *)k1, nr, head_pos);
	HIP_TRY(hipGetLastError());
	HIP_TRY(rocprim::inclusive_scan(ctx->pam_tmp.p, t1, head_pos, run_start, N, rocprim::maximum<uint32_t>(), ctx->stream));
	hipLaunchKernelGGL(k_amp_verify, dim3(grid_w), dim3(64*AMP_WAVES), 0, ctx->stream, (const uint4 *)S.planes.p, (const uint64_t *)S.d_blk_off.p,
		(const uint4 *)ctx->pam_iv.p, (const uint4 *)ctx->pam_stat.p, (const uint32_t *)o1, (const uint32_t *)run_start, nr, rep, n_flag);
	HIP_TRY(hipGetLastError());
	uint32_t flagged = 0;
	HIP_TRY(hipMemcpyAsync(&flagged, n_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));                                   // (iv is read by now)
	// ---- 3. two spellings under one key: the records that differ from their run's first, grouped by their bytes
	if(flagged){
		std::vector<uint32_t> h_rep(N), list;
		HIP_TRY(hipMemcpyAsync(h_rep.data(), rep, N*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		std::vector<uint64_t> off;
		uint64_t bytes = 0;
		for(uint32_t k = 0;k < nr;++k) if(h_rep[k] == AMP_UNRESOLVED){ list.push_back(k); off.push_back(bytes); bytes += (iv[k].z + 1u)/2u; }
		if(bytes >= (1ull << 40)){ g_err = "pcr_pool_amplicons: the spellings to resolve reach 2^40 bytes"; return PCR_ERR_CAPACITY; }
		if((rc = ctx->pam_packed.ensure(bytes + 16)) != PCR_OK) return rc;
		// (class_rec[] and class_off[] are free until step 4)
		HIP_TRY(hipMemcpyAsync(class_rec, list.data(), list.size()*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(hipMemcpyAsync(class_off, off.data(), off.size()*sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
		const uint32_t nl = (uint32_t)list.size();
		hipLaunchKernelGGL(k_amp_extract, dim3(std::min<unsigned>((nl + AMP_BLOCK_RECORDS - 1)/AMP_BLOCK_RECORDS, ctx->n_cu*16)), dim3(64*AMP_WAVES), 0, ctx->stream,
			(const uint4 *)S.planes.p, (const uint64_t *)S.d_blk_off.p, (const uint4 *)ctx->pam_iv.p, (const uint4 *)ctx->pam_stat.p,
			(const uint32_t *)class_rec, (const uint64_t *)class_off, nl, ctx->pam_packed.p);
		HIP_TRY(hipGetLastError());
		std::vector<uint8_t> text(bytes);
		if(bytes) HIP_TRY(hipMemcpyAsync(text.data(), ctx->pam_packed.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));
		std::unordered_map<std::string, uint32_t> first_of;                       // length + bytes -> the lowest record that spells them
		for(size_t i = 0;i < list.size();++i){
			const uint32_t k = list[i], len = iv[k].z;
			std::string s((const char *)&len, sizeof(len));
			s.append((const char *)text.data() + off[i], (len + 1u)/2u);
			h_rep[k] = first_of.emplace(std::move(s), k).first->second;           // (list is ascending)
		}
		HIP_TRY(hipMemcpyAsync(rep, h_rep.data(), N*sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(hipStreamSynchronize(ctx->stream));                               // (h_rep is a local)
	}
	// ---- 4. copies, class ids by first appearance, distinct sequences, the records, the classes' lengths and offsets
	hipLaunchKernelGGL(k_amp_count, dim3(grid_t), dim3(256), 0, ctx->stream, (const uint4 *)ctx->pam_iv.p, (const uint32_t *)rep, nr, copies, head, k0);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemsetAsync(head + N, 0, sizeof(uint32_t), ctx->stream));
	HIP_TRY(rocprim::exclusive_scan(ctx->pam_tmp.p, t2, head, cls, uint32_t(0), N + 1, rocprim::plus<uint32_t>(), ctx->stream));
	HIP_TRY(rocprim::radix_sort_keys(ctx->pam_tmp.p, t3, k0, k1, nr, 0, 64, ctx->stream));
	hipLaunchKernelGGL(k_amp_seqs, dim3(grid_t), dim3(256), 0, ctx->stream, (const uint64_t *)k1, nr, n_seq);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_amp_info, dim3(grid_t), dim3(256), 0, ctx->stream, (const uint4 *)ctx->pam_iv.p, (const uint4 *)ctx->pam_stat.p, (const uint32_t *)rep,
		(const uint32_t *)cls, (const uint32_t *)copies, (const uint32_t *)n_seq, nr, ctx->pam_info.p, class_rec, class_len, class_bytes);
	HIP_TRY(hipGetLastError());
	uint32_t n_classes = 0;
	HIP_TRY(hipMemcpyAsync(&n_classes, cls + N, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
	if(info) HIP_TRY(hipMemcpyAsync(info, ctx->pam_info.p, N*sizeof(pcr_amplicon_info), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	const size_t C = n_classes;                                                   // (>= 1; the scan below reads class_bytes[0 .. C])
	HIP_TRY(hipMemsetAsync(class_bytes + C, 0, sizeof(uint32_t), ctx->stream));
	HIP_TRY(rocprim::exclusive_scan(ctx->pam_tmp.p, t4, class_bytes, class_off, uint64_t(0), C + 1, rocprim::plus<uint64_t>(), ctx->stream));
	uint64_t total = 0;
	HIP_TRY(hipMemcpyAsync(&total, class_off + C, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	if(total >= (1ull << 40)){ g_err = "pcr_pool_amplicons: the packed amplicons reach 2^40 bytes"; return PCR_ERR_CAPACITY; }
	if(packed_bytes) *packed_bytes = total;
	if(C <= class_cap){
		HIP_TRY(hipMemcpyAsync(class_byte_offset, class_off, C*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(hipMemcpyAsync(class_length, class_len, C*sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
	}
	// ---- 5. the unique amplicons
	if(packed4 && total && total <= packed_cap){
		if((rc = ctx->pam_packed.ensure(total + 16)) != PCR_OK) return rc;
		hipLaunchKernelGGL(k_amp_extract, dim3(std::min<unsigned>((n_classes + AMP_BLOCK_RECORDS - 1)/AMP_BLOCK_RECORDS, ctx->n_cu*16)), dim3(64*AMP_WAVES), 0, ctx->stream,
			(const uint4 *)S.planes.p, (const uint64_t *)S.d_blk_off.p, (const uint4 *)ctx->pam_iv.p, (const uint4 *)ctx->pam_stat.p,
			(const uint32_t *)class_rec, (const uint64_t *)class_off, n_classes, ctx->pam_packed.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(packed4, ctx->pam_packed.p, total, hipMemcpyDeviceToHost, ctx->stream));
	}
	HIP_TRY(hipStreamSynchronize(ctx->stream));
	return (int64_t)n_classes;
}

} // extern "C"

// Assay-list writers (scope row f-4): the bytes `pcramp` writes to its output file, text and JSON
// (main.cpp:131-163, 440-443, 460-462, 504-519, 950-1113, 1132-1264, 1326-1400; PCR::write / write_json,
// assay.h:288-375).  Host-only; included at the end of pcr_device.hip.
//
// Number formatting is the reference's: std::ostream defaults, i.e. "%g" with six significant digits for float and
// double, plain decimal for integers.  `endl` is "\n".
namespace {

struct Out {
	std::string s;
	Out &operator<<(const char *t) { s += t; return *this; }
	Out &operator<<(const std::string &t) { s += t; return *this; }
	Out &operator<<(char c) { s.push_back(c); return *this; }
	Out &operator<<(unsigned v) { char b[32]; snprintf(b, sizeof(b), "%u", v); s += b; return *this; }
	Out &operator<<(unsigned long v) { char b[32]; snprintf(b, sizeof(b), "%lu", v); s += b; return *this; }
	Out &operator<<(float v) { char b[64]; snprintf(b, sizeof(b), "%g", (double)v); s += b; return *this; }
	Out &operator<<(double v) { char b[64]; snprintf(b, sizeof(b), "%g", v); s += b; return *this; }
};

int64_t emit(const Out &o, char *out, uint64_t cap)
{
	if(out && cap){
		const size_t n = std::min<size_t>(o.s.size(), cap);
		memcpy(out, o.s.data(), n);
		if(n < cap) out[n] = 0;
	}
	return (int64_t)o.s.size();
}

const char RULE[] = "###########################################################################################";

// operator<<(ostream&, const Word&) / Word::str (word.cpp:296-320, word.h:649-666): the slots from start() to stop()
std::string word_str(const uint64_t w[2], bool lower)
{
	static const char sym[17] = "-ACMGRSVTWYHKDBN";       // bits_to_base, base_table.h:78-122 (A=1 C=2 G=4 T=8, unions; 0 = EOS)
	const Planes p = pcrhost::planes_of_word(w);
	std::string r;
	for(int k = pcrhost::planes_start(p);k <= pcrhost::planes_stop(p);++k){
		const char c = sym[pcrhost::planes_nibble(p, k) & 15];
		r.push_back(lower ? (char)tolower(c) : c);             // tolower(const string&), options.cpp:1338
	}
	return r;
}

// the reuse test of PCR::write / write_json (assay.h:309-323): an oligo some pooled oligo overlaps completely
void reused(const pcr_pair *a, const pcr_pair *pool, uint32_t n_pool, bool &lower_f, bool &lower_r)
{
	lower_f = lower_r = false;
	const Planes F = pcrhost::planes_of_word(a->f.w), R = pcrhost::planes_of_word(a->r.w);
	for(uint32_t i = 0;i < n_pool;++i){
		const Planes pf = pcrhost::planes_of_word(pool[i].f.w), pr = pcrhost::planes_of_word(pool[i].r.w);
		if(std::max(pcrhost::max_overlap(F, pf), pcrhost::max_overlap(F, pr)) == 1.0f) lower_f = true;
		if(std::max(pcrhost::max_overlap(R, pf), pcrhost::max_overlap(R, pr)) == 1.0f) lower_r = true;
	}
}

void write_oligos(Out &o, const pcr_pair *a, const pcr_pair *pool, uint32_t n_pool, bool json, bool multiplex)
{
	const double df = pcrhost::planes_degeneracy(pcrhost::planes_of_word(a->f.w));
	const double dr = pcrhost::planes_degeneracy(pcrhost::planes_of_word(a->r.w));
	bool lf = false, lr = false;
	if(multiplex) reused(a, pool, n_pool, lf, lr);
	if(!json){                                                   // assay.h:288-293, 304-343
		o << word_str(a->f.w, lf) << '\t' << word_str(a->r.w, lr) << "\tD(F)=" << df << ";D(R)=" << dr;
		return;
	}
	// write_json never lower-cases the sequence, it reports "recycled" (assay.h:345-375)
	o << "\t\t\t\"forward primer\":{\n" << "\t\t\t\t\"sequence\":\"" << word_str(a->f.w, false) << "\",\n"
	  << "\t\t\t\t\"degeneracy\":" << df;
	if(multiplex) o << ",\n\t\t\t\t\"recycled\":" << (lf ? "True" : "False") << "\n\t\t\t},\n";
	else o << "\n\t\t\t},\n";
	o << "\t\t\t\"reverse primer\":{\n" << "\t\t\t\t\"sequence\":\"" << word_str(a->r.w, false) << "\",\n"
	  << "\t\t\t\t\"degeneracy\":" << dr;
	if(multiplex) o << ",\n\t\t\t\t\"recycled\":" << (lr ? "True" : "False") << "\n\t\t\t},\n";
	else o << "\n\t\t\t},\n";
}

// sequence_summary (main.cpp:1326-1400)
void summary(Out &o, const char *prefix, const uint64_t *len, uint32_t n, bool json)
{
	if(!json) o << prefix << " Number of sequences = " << n << '\n';
	else o << "\t\"" << prefix << "\":{\n" << "\t\t\"number of sequences\":" << n;
	if(n == 0){
		if(json) o << "\n\t},\n";
		return;
	}
	float ave = 0.0f, stdev = 0.0f;
	unsigned mn = (unsigned)len[0], mx = (unsigned)len[0];
	for(uint32_t i = 0;i < n;++i){
		const unsigned l = (unsigned)len[i];
		ave += l;
		mn = std::min(mn, l); mx = std::max(mx, l);
	}
	ave /= n;
	for(uint32_t i = 0;i < n;++i){
		const float tmp = (unsigned)len[i] - ave;
		stdev += tmp*tmp;
	}
	stdev = (n > 1) ? sqrtf(stdev/(n - 1)) : 0.0f;
	if(!json){
		o << prefix << " Min sequence length = " << mn << '\n';
		o << prefix << " Max sequence length = " << mx << '\n';
		o << prefix << " Average sequence length = " << ave << '\n';
		o << prefix << " Stdev sequence length = " << stdev << '\n';
	}
	else{
		o << ",\n\t\t\"min sequence length\":" << mn << ",\n" << "\t\t\"max sequence length\":" << mx << ",\n"
		  << "\t\t\"average sequence length\":" << ave << ",\n" << "\t\t\"stdev sequence length\":" << stdev << "\n\t},\n";
	}
}

// version, command line and seed (main.cpp:131-163): the lines the reference writes before it reads its inputs
void write_preamble(Out &o, bool json, int argc, const char *const *argv, uint32_t seed)
{
	if(!json){                                                   // main.cpp:132-147
		o << "PCRamp version 0.3\n" << "Command line:";
		for(int i = 0;i < argc;++i) o << ' ' << argv[i];
		o << '\n' << "Random number seed = " << (unsigned)seed << '\n';
	}
	else{                                                        // main.cpp:148-160
		o << "{\n\t\"program\":\"PCRamp\",\n" << "\t\"version\":\"0.3\",\n\t" << "\"command line\":\"" << argv[0];
		for(int i = 1;i < argc;++i) o << ' ' << argv[i];
		o << "\",\n\t\"seed\":" << (unsigned)seed << ',' << '\n';
	}
}

inline bool bit(const uint64_t *w, uint32_t i) { return w && ((w[i >> 6] >> (i & 63)) & 1ull); }

} // namespace

extern "C" {

int64_t pcr_format_oligos(const pcr_pair *assay, const pcr_pair *pool, uint32_t n_pool, int json, int use_multiplex, char *out, uint64_t cap)
{
	if(!assay || (n_pool && !pool)){ g_err = "pcr_format_oligos: bad argument"; return PCR_ERR_ARG; }
	Out o;
	write_oligos(o, assay, pool, n_pool, json != 0, use_multiplex != 0);
	return emit(o, out, cap);
}

int64_t pcr_format_header(const pcr_output *f, int argc, const char *const *argv, uint32_t seed, char *out, uint64_t cap)
{
	if(!f || argc < 1 || !argv){ g_err = "pcr_format_header: bad argument"; return PCR_ERR_ARG; }
	Out o;
	write_preamble(o, f->json != 0, argc, argv, seed);
	summary(o, "target sequence summary", f->target_lengths, f->n_target, f->json != 0);           // main.cpp:440
	summary(o, "background sequence summary", f->background_lengths, f->n_background, f->json != 0);   // main.cpp:443
	if(f->json) o << "\t\"assays\":[\n";                           // main.cpp:460-462
	return emit(o, out, cap);
}

int64_t pcr_format_preamble(int json, int argc, const char *const *argv, uint32_t seed, char *out, uint64_t cap)
{
	if(argc < 1 || !argv){ g_err = "pcr_format_preamble: bad argument"; return PCR_ERR_ARG; }
	Out o;
	write_preamble(o, json != 0, argc, argv, seed);
	return emit(o, out, cap);
}

int64_t pcr_format_iteration(const pcr_output *f, uint32_t assay_iteration, uint32_t major_id, uint32_t minor_id, uint32_t targets_remaining,
	char *out, uint64_t cap)
{
	if(!f){ g_err = "pcr_format_iteration: bad argument"; return PCR_ERR_ARG; }
	Out o;
	if(f->json){                                                 // main.cpp:504-511
		if(assay_iteration > 1) o << ",\n";
		o << "\t\t{\n\t\t\t\"id\":" << major_id << '.' << minor_id << ",\n";
	}
	else o << RULE << '\n' << "# Attempting to detect " << targets_remaining << " remaining targets" << '\n';   // main.cpp:515-519
	return emit(o, out, cap);
}

int64_t pcr_format_assay(const pcr_output *f, const pcr_assay_record *r, const pcr_pair *pool, uint32_t n_pool, char *out, uint64_t cap)
{
	if(!f || !r || (n_pool && !pool)){ g_err = "pcr_format_assay: bad argument"; return PCR_ERR_ARG; }
	Out o;
	if(!f->json){                                                // main.cpp:950-961
		o << "# Assay " << r->major_id << '.' << r->minor_id << " has target coverage score = " << r->target_coverage
		  << " (" << (r->target_coverage*100.0f)/r->active_target_norm << "% of active) and background coverage score = "
		  << r->background_coverage << " ("
		  << ((r->num_active_background == 0) ? 0.0f : (r->background_coverage*100.0f)/r->active_background_norm)
		  << "% of active)" << '\n';
		o << "ASSAY." << r->major_id << '.' << r->minor_id << '\t';
		write_oligos(o, &r->assay, pool, n_pool, false, f->use_multiplex != 0);
		o << '\n';
		for(uint32_t i = 0;i < f->n_target;++i){ if(bit(r->target_match, i)) o << "T-" << f->target_deflines[i] << '\n'; }           // main.cpp:1040-1052
		for(uint32_t i = 0;i < f->n_background;++i){ if(bit(r->background_match, i)) o << "B-" << f->background_deflines[i] << '\n'; }
		return emit(o, out, cap);
	}
	write_oligos(o, &r->assay, pool, n_pool, true, f->use_multiplex != 0);
	o << "\t\t\t\"target matches\":[\n";                         // main.cpp:1056-1109
	bool first = true;
	for(uint32_t i = 0;i < f->n_target;++i){
		if(!bit(r->target_match, i)) continue;
		o << (first ? "\t\t\t\t\"" : ",\n\t\t\t\t\"") << f->target_deflines[i] << "\"";
		first = false;
	}
	o << "\n\t\t\t],\n";
	o << "\t\t\t\"background matches\":[";
	first = true;
	for(uint32_t i = 0;i < f->n_background;++i){
		if(!bit(r->background_match, i)) continue;
		o << (first ? "\n\t\t\t\t\"" : ",\n\t\t\t\t\"") << f->background_deflines[i] << "\"";
		first = false;
	}
	o << (first ? "]\n\t\t}" : "\n\t\t\t]\n\t\t}");
	return emit(o, out, cap);
}

int64_t pcr_format_footer(const pcr_output *f, const uint8_t *target_active, const uint64_t *total_background, char *out, uint64_t cap)
{
	if(!f || (f->n_target && !target_active)){ g_err = "pcr_format_footer: bad argument"; return PCR_ERR_ARG; }
	Out o;
	if(f->json) o << "\n\t],\n";                                 // main.cpp:1132-1134
	unsigned undetected = 0, cross = 0;
	for(uint32_t i = 0;i < f->n_target;++i) undetected += target_active[i] ? 1u : 0u;
	for(uint32_t i = 0;i < f->n_background;++i) cross += bit(total_background, i) ? 1u : 0u;
	if(!f->json){                                                // main.cpp:1166-1202
		o << RULE << '\n';
		if(undetected == 0) o << "# Detected all targets" << '\n';
		else{
			o << "# Failed to detect a total of " << undetected << " targets" << '\n';
			o << "# The following targets were *not* detected by any assay" << '\n';
			for(uint32_t i = 0;i < f->n_target;++i){ if(target_active[i]) o << "-T-" << f->target_deflines[i] << '\n'; }
		}
		o << RULE << '\n' << "# Cross reacted with a total of " << cross << " background sequences" << '\n';
		for(uint32_t i = 0;i < f->n_background;++i){ if(bit(total_background, i)) o << "+B-" << f->background_deflines[i] << '\n'; }
		return emit(o, out, cap);
	}
	o << "\t\"unmatched targets\":[";                            // main.cpp:1204-1261
	if(undetected == 0) o << "],\n";
	else{
		bool first = true;
		for(uint32_t i = 0;i < f->n_target;++i){
			if(!target_active[i]) continue;
			o << (first ? "\t\t\"" : ",\n\t\t\"") << f->target_deflines[i] << "\"";
			first = false;
		}
		o << "\n\t],\n";
	}
	o << "\t\"total number of background matches\":" << cross << ",\n";
	if(cross > 0){
		o << "\t\"background matches\":[\n";
		bool first = true;
		for(uint32_t i = 0;i < f->n_background;++i){
			if(!bit(total_background, i)) continue;
			o << (first ? "\t\t\"" : ",\n\t\t\"") << f->background_deflines[i] << "\"";
			first = false;
		}
	}
	else o << "\t\"background matches\":[]";
	o << "\n}" << '\n';
	return emit(o, out, cap);
}

} // extern "C"

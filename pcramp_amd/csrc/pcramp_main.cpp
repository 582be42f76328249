// pcramp_main.cpp -- the `pcramp` program: the reference's command line (options.cpp), its FASTA ingest (main.cpp:253-436,
// parse_fasta.cpp, Sequence::defline) and its output file, with the design loop behind pcr_design (scope row f-8).
//
// Host C++17 over include/pcramp_hip.h and zlib; no HIP of its own.  One rank: the MPI modes of the reference are not offered
// here (they are pcr_shard_targets / pcr_design_trial_ranks of the library).  The GPU is first touched once every input has
// been read: quits and ingest errors end the program without it.
#include "pcramp_hip.h"

#include <getopt.h>
#include <sys/stat.h>
#include <dirent.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

// ---- options (pcramp.h:14-52 defaults, options.cpp:161-214 switches)

enum Verbosity { SILENT, VERBOSE, EVERYTHING };

struct Options {
	Verbosity verbosity = VERBOSE;
	bool json = false;
	std::vector<std::string> target_files, background_files, target_dirs, background_dirs;
	std::string target_prefix, background_prefix, input_prefix, output;
	unsigned degen = 1, num_trial = 1000, num_assay = 100, seed = 0, threads = 0;
	int target_amp_min = 80, target_amp_max = 200, background_amp_min = 0, background_amp_max = 2000;
	int target_size_min = 0, target_size_max = INT_MAX, background_size_min = 0, background_size_max = INT_MAX;
	int primer_min = 18, primer_max = 25;
	float tm_min = 50.0f, tm_max = 75.0f, max_hairpin = 40.0f, max_dimer = 40.0f, primer_strand = 900.0e-9f, salt = 0.05f;
	float target_weight = 1.0f, background_weight = 1.0f;          // accepted and checked; nothing reads them (nor in the reference)
	float target_search = 0.9f, background_search = 0.9f, target_threshold = 1.0f, background_threshold = 0.8f;
	float min_target_cover = 0.0f, max_background_cover = 0.0f;
	unsigned pack_max_degen = 256;
	float pack_min_gc = 0.0f, pack_max_gc = 1.0f;
	std::vector<std::string> target_ignore, background_ignore;
	bool taq_mama = false, top_down = false, normalize_target = false, normalize_background = false, optimize_5 = false, optimize_3 = false;
	bool json_config = false;                                      // --json / --json.root were given
	// groups (-T / -B): group name (the directory, or the file named on its own) -> its FASTA files
	std::map<std::string, std::vector<std::string>> target_groups, background_groups;
};

enum Status { RUN, QUIT, REFUSE };

void usage()
{
	fprintf(stderr,
		"PCRamp version 0.3\n"
		"Usage:\n"
		"\t-t <target fasta file>\n"
		"\t-T <root directory of target subdirectories>\n"
		"\t[--T.prefix <directory prefix for target genomes>]\n"
		"\t[-b <background fasta file>]\n"
		"\t[-B <root directory of background subdirectories>]\n"
		"\t[--B.prefix <directory prefix for background genomes>]\n"
		"\t-o <output file>\n"
		"\t[--o.text (output results as [poorly] structured text)]\n"
		"\t[--o.json (output results in JSON format)]\n"
		"\t[-d <max degeneracy> (default is 1)]\n"
		"\t[--trial <number of trials (default is 1000)>]\n"
		"\t[--seed <random number seed> (default is time-based)]\n"
		"\t[--thread <maximum number of threads> (accepted; the design runs on one GPU)]\n"
		"\t[--salt <salt concentration> (default is 0.05)\n"
		"\t[--primer.hairpin <max oligo hairpin Tm> (default is 40)\n"
		"\t[--primer.dimer <max oligo hetero/homo-dimer Tm> (default is 40)\n"
		"\t[--count <total number of amplicons to produce> (default is 100)]\n"
		"\t[--optimize.top-down Search using maximally degenerate inital primer oligos (default is bottom up)]\n"
		"\t[--optimize.5 (enable 5' primer search to optimize coverage)]\n"
		"\t[--no-optimize.5 (disable 5' primer search to optimize coverage; default)]\n"
		"\t[--optimize.3 (enable 3' primer search to optimize coverage)]\n"
		"\t[--no-optimize.3 (disable 3' primer search to optimize coverage; default)]\n"
		"\t[-v <verbosity level: silent, verbose, everything>]\n"
		"\t[--target.amplicon.min <minimum amplicon length> (default is 80)]\n"
		"\t[--target.amplicon.max <maximum amplicon length> (default is 200)]\n"
		"\t[--target.threshold <target detection threshold> (default is 1)]\n"
		"\t[--target.search <target search multiplier> (default is 0.9)]\n"
		"\t[--target.cover <minimum per primer pair coverage> (default is 0)]\n"
		"\t[--target.ignore <defline key word to exclude a sequence>]\n"
		"\t[--target.normalize (normalize target weights per fasta file)]\n"
		"\t[--target.size.min <length> (minimum input target length in bp)]\n"
		"\t[--target.size.max <length> (maximum input target length in bp)]\n"
		"\t[--background.amplicon.min <minimum amplicon length>]\n"
		"\t[--background.amplicon.max <maximum amplicon length>]\n"
		"\t[--background.threshold <background detection threshold> (default is 0.8)]\n"
		"\t[--background.search <background search multiplier> (default is 0.9)]\n"
		"\t[--background.cover <maximum per primer pair coverage> (default is 0)]\n"
		"\t[--background.ignore <defline key word to exclude a sequence>]\n"
		"\t[--background.normalize (normalize background weights per fasta file)]\n"
		"\t[--background.size.min <length> (minimum input background length in bp)]\n"
		"\t[--background.size.max <length> (maximum input background length in bp)]\n"
		"\t[--primer.size.min <minimum primer length> (default is 18)]\n"
		"\t[--primer.size.max <maximum primer length> (default is 25)]\n"
		"\t[--primer.tm.min <minimum primer melting temperature> (default is 50)]\n"
		"\t[--primer.tm.max <maximum primer melting temperature> (default is 75)]\n"
		"\t[--primer.strand <primer strand concentration> (default is 9e-07)]\n"
		"\t[--primer.taq-mama (use Taq MAMA rules for terminal primer mismatches; default is false)]\n"
		"\t[--pack.degen.max <max degen when packing words> (default is 256)]\n"
		"\t[--pack.gc.max <max fractional GC content when packing words> (default is 1, disabled)]\n"
		"\t[--pack.gc.min <min fractional GC content when packing words> (default is 0, disabled)]\n"
		"\t[--input.prefix <directory prefix for both target and background input genomes>]\n");
}

std::string lower(std::string s)
{
	for(char &c : s) c = (char)tolower((unsigned char)c);
	return s;
}

// make_set (pcramp.h:239-247): sorted, duplicates removed
void make_set(std::vector<std::string> &v)
{
	std::sort(v.begin(), v.end());
	v.erase(std::unique(v.begin(), v.end()), v.end());
}

// find_file_extension (options.cpp:1440-1457): the FIRST occurrence of an extension must end the path
bool fasta_extension(const std::string &path)
{
	static const char *const ext[] = {".fna", ".fna.gz", ".fasta", ".fasta.gz", ".fa", ".fa.gz"};
	for(const char *e : ext){
		const size_t at = path.find(e);
		if(at != std::string::npos && at + strlen(e) == path.size()) return true;
	}
	return false;
}

// find_groups (options.cpp:1349-1438): every directory under `path` that holds FASTA files is one group of them, a FASTA file
// named on its own a group of one.  false = the path is neither (the "Invalid path" quit).  A group's files are kept in byte-wise
// sorted order here (the reference appends them in readdir order through an unordered_multimap: DESIGN.md section 5).
bool find_groups(const std::string &path, std::map<std::string, std::vector<std::string>> &groups)
{
	struct stat st;
	if(stat(path.c_str(), &st) != 0) return false;
	if(S_ISREG(st.st_mode)){
		if(!fasta_extension(path)) return false;
		groups[path].push_back(path);
		return true;
	}
	if(!S_ISDIR(st.st_mode)) return false;
	DIR *dp = opendir(path.c_str());
	if(!dp) return false;
	std::vector<std::string> subdirs;
	while(const struct dirent *e = readdir(dp)){
		if(e->d_ino == 0 || !strcmp(e->d_name, ".") || !strcmp(e->d_name, "..")) continue;
		const std::string name = path + '/' + e->d_name;
		struct stat es;
		if(stat(name.c_str(), &es) != 0) continue;
		if(S_ISDIR(es.st_mode)) subdirs.push_back(name);
		else if(S_ISREG(es.st_mode) && fasta_extension(name)) groups[path].push_back(name);
	}
	closedir(dp);
	std::sort(subdirs.begin(), subdirs.end());
	for(const std::string &d : subdirs)
		if(!find_groups(d, groups)) return false;
	return true;
}

bool verbosity_of(std::string s, Verbosity &v)
{
	s = lower(s);
	if(s == "silent") v = SILENT;
	else if(s == "verbose") v = VERBOSE;
	else if(s == "everything") v = EVERYTHING;
	else return false;
	return true;
}

// Options::load (options.cpp:100-1001) restated: the same switches through getopt_long (so the same abbreviations, "=value"
// forms and argv permutation), the same checks in the same order.  QUIT = the reference's opt.quit (a message or the usage on
// stderr, no output file, EXIT_SUCCESS); REFUSE = --json / --json.root, which this program does not read.
Status load_options(int argc, char **argv, Options &o)
{
	enum {
		TARGET_AMP_MIN = 256, TARGET_AMP_MAX, PRIMER_MIN, PRIMER_MAX, BACKGROUND_AMP_MIN, BACKGROUND_AMP_MAX, SEED, TARGET_WEIGHT,
		BACKGROUND_WEIGHT, TARGET_THRESHOLD, BACKGROUND_THRESHOLD, TARGET_COVER, BACKGROUND_COVER, TAQ_MAMA, TRIAL, PACK_DEGEN,
		PACK_GC_MIN, PACK_GC_MAX, COUNT, TARGET_SEARCH, TOP_DOWN, TARGET_IGNORE, BACKGROUND_IGNORE, TM_MIN, TM_MAX, STRAND, SALT,
		HAIRPIN, DIMER, TARGET_NORMALIZE, BACKGROUND_NORMALIZE, THREAD, TARGET_SIZE_MIN, TARGET_SIZE_MAX, BACKGROUND_SIZE_MIN,
		BACKGROUND_SIZE_MAX, BACKGROUND_SEARCH, OPT5, NO_OPT5, OPT3, NO_OPT3, JSON_FILE, JSON_ROOT, TARGET_PREFIX, BACKGROUND_PREFIX,
		INPUT_PREFIX, OUT_TEXT, OUT_JSON
	};
	static const struct option longs[] = {
		{"target.amplicon.min", required_argument, nullptr, TARGET_AMP_MIN}, {"target.amplicon.max", required_argument, nullptr, TARGET_AMP_MAX},
		{"primer.size.min", required_argument, nullptr, PRIMER_MIN}, {"primer.size.max", required_argument, nullptr, PRIMER_MAX},
		{"background.amplicon.min", required_argument, nullptr, BACKGROUND_AMP_MIN},
		{"background.amplicon.max", required_argument, nullptr, BACKGROUND_AMP_MAX},
		{"seed", required_argument, nullptr, SEED}, {"target.weight", required_argument, nullptr, TARGET_WEIGHT},
		{"background.weight", required_argument, nullptr, BACKGROUND_WEIGHT},
		{"target.threshold", required_argument, nullptr, TARGET_THRESHOLD}, {"background.threshold", required_argument, nullptr, BACKGROUND_THRESHOLD},
		{"target.cover", required_argument, nullptr, TARGET_COVER}, {"background.cover", required_argument, nullptr, BACKGROUND_COVER},
		{"primer.taq-mama", no_argument, nullptr, TAQ_MAMA}, {"trial", required_argument, nullptr, TRIAL},
		{"pack.degen.max", required_argument, nullptr, PACK_DEGEN}, {"pack.gc.min", required_argument, nullptr, PACK_GC_MIN},
		{"pack.gc.max", required_argument, nullptr, PACK_GC_MAX}, {"count", required_argument, nullptr, COUNT},
		{"target.search", required_argument, nullptr, TARGET_SEARCH}, {"optimize.top-down", no_argument, nullptr, TOP_DOWN},
		{"target.ignore", required_argument, nullptr, TARGET_IGNORE}, {"background.ignore", required_argument, nullptr, BACKGROUND_IGNORE},
		{"primer.tm.min", required_argument, nullptr, TM_MIN}, {"primer.tm.max", required_argument, nullptr, TM_MAX},
		{"primer.strand", required_argument, nullptr, STRAND}, {"salt", required_argument, nullptr, SALT},
		{"primer.hairpin", required_argument, nullptr, HAIRPIN}, {"primer.dimer", required_argument, nullptr, DIMER},
		{"target.normalize", no_argument, nullptr, TARGET_NORMALIZE}, {"background.normalize", no_argument, nullptr, BACKGROUND_NORMALIZE},
		{"thread", required_argument, nullptr, THREAD},
		{"target.size.min", required_argument, nullptr, TARGET_SIZE_MIN}, {"target.size.max", required_argument, nullptr, TARGET_SIZE_MAX},
		{"background.size.min", required_argument, nullptr, BACKGROUND_SIZE_MIN},
		{"background.size.max", required_argument, nullptr, BACKGROUND_SIZE_MAX},
		{"background.search", required_argument, nullptr, BACKGROUND_SEARCH},
		{"optimize.5", no_argument, nullptr, OPT5}, {"no-optimize.5", no_argument, nullptr, NO_OPT5},
		{"optimize.3", no_argument, nullptr, OPT3}, {"no-optimize.3", no_argument, nullptr, NO_OPT3},
		{"json", required_argument, nullptr, JSON_FILE}, {"json.root", required_argument, nullptr, JSON_ROOT},
		{"target.prefix", required_argument, nullptr, TARGET_PREFIX}, {"T.prefix", required_argument, nullptr, TARGET_PREFIX},
		{"background.prefix", required_argument, nullptr, BACKGROUND_PREFIX}, {"B.prefix", required_argument, nullptr, BACKGROUND_PREFIX},
		{"input.prefix", required_argument, nullptr, INPUT_PREFIX},
		{"o.text", no_argument, nullptr, OUT_TEXT}, {"o.json", no_argument, nullptr, OUT_JSON},
		{nullptr, 0, nullptr, 0}};
	auto quit = [](const char *msg) { fprintf(stderr, "%s\n", msg); return QUIT; };
	bool print_usage = argc <= 1;
	opterr = 0;
	int c;
	while((c = getopt_long(argc, argv, "t:T:b:B:o:d:v:?h", longs, nullptr)) != -1){
		const char *a = optarg;
		switch(c){
		case 't': o.target_files.push_back(a); break;
		case 'T': o.target_dirs.push_back(a); break;
		case 'b': o.background_files.push_back(a); break;
		case 'B': o.background_dirs.push_back(a); break;
		case 'o': o.output = a; break;
		case 'd': o.degen = (unsigned)abs(atoi(a)); break;
		case 'v': if(!verbosity_of(a, o.verbosity)) return quit("Please enter a valid verbosity flag: \"silent\", \"verbose\", \"everything\""); break;
		case 'h': case '?': print_usage = true; break;
		case TARGET_AMP_MIN: if((o.target_amp_min = atoi(a)) < 0) return quit("Please specify a target.amplicon.min >= 0"); break;
		case TARGET_AMP_MAX: if((o.target_amp_max = atoi(a)) < 0) return quit("Please specify a target.amplicon.max >= 0"); break;
		case PRIMER_MIN: if((o.primer_min = atoi(a)) < 0) return quit("Please specify a primer.min >= 0"); break;
		case PRIMER_MAX: if((o.primer_max = atoi(a)) < 0) return quit("Please specify a primer.max >= 0"); break;
		case BACKGROUND_AMP_MIN: if((o.background_amp_min = atoi(a)) < 0) return quit("Please specify a background.amplicon.min >= 0"); break;
		case BACKGROUND_AMP_MAX: if((o.background_amp_max = atoi(a)) < 0) return quit("Please specify a background.amplicon.max >= 0"); break;
		case SEED: o.seed = (unsigned)abs(atoi(a)); break;
		case TARGET_WEIGHT: if((o.target_weight = atof(a)) < 1.0) return quit("Please specify a valid target.weight value (>= 1.0)"); break;
		case BACKGROUND_WEIGHT: if((o.background_weight = atof(a)) < 0.0f) return quit("Please specify a valid background.weight value (>= 0.0)"); break;
		case TARGET_THRESHOLD:
			o.target_threshold = atof(a);
			if(o.target_threshold < 0.0f || o.target_threshold > 1.0f) return quit("Please specify a valid target.threshold value (0 <= PCR <= 1)");
			break;
		case BACKGROUND_THRESHOLD:
			o.background_threshold = atof(a);
			if(o.background_threshold < 0.0f || o.background_threshold > 1.0f) return quit("Please specify a valid background.threshold value (0 <= PCR <= 1)");
			break;
		case TARGET_COVER: if((o.min_target_cover = atof(a)) < 0.0f) return quit("Please specify a valid target.cover value (>= 0)"); break;
		case BACKGROUND_COVER: if((o.max_background_cover = atof(a)) < 0.0f) return quit("Please specify a valid background.cover value (>= 0)"); break;
		case TAQ_MAMA: o.taq_mama = true; break;
		case TRIAL: if((o.num_trial = (unsigned)fabs(atof(a))) == 0) return quit("Please enter --trial > 0"); break;   // a float: "1e5" works
		case PACK_DEGEN: if((o.pack_max_degen = (unsigned)abs(atoi(a))) == 0) return quit("Please enter --pack.max_degen > 0"); break;
		case PACK_GC_MIN:
			o.pack_min_gc = atof(a);
			if(o.pack_min_gc < 0.0f || o.pack_min_gc > 1.0f) return quit("Please enter --pack.min_gc >= 0 and <= 1.0");
			break;
		case PACK_GC_MAX:
			o.pack_max_gc = atof(a);
			if(o.pack_max_gc < 0.0f || o.pack_max_gc > 1.0f) return quit("Please enter --pack.max_gc >= 0 and <= 1.0");
			break;
		case COUNT: if((o.num_assay = (unsigned)abs(atoi(a))) == 0) return quit("Please enter --count >= 1"); break;
		case TARGET_SEARCH:
			o.target_search = atof(a);
			if(o.target_search <= 0.0 || o.target_search > 1.0) return quit("Please enter 0 < target.search <= 1");
			break;
		case BACKGROUND_SEARCH:
			o.background_search = atof(a);
			if(o.background_search <= 0.0 || o.background_search > 1.0) return quit("Please enter 0 < background.search <= 1");
			break;
		case TOP_DOWN: o.top_down = true; break;
		case TARGET_IGNORE: o.target_ignore.push_back(lower(a)); break;
		case BACKGROUND_IGNORE: o.background_ignore.push_back(lower(a)); break;
		case TM_MIN: o.tm_min = atof(a); break;
		case TM_MAX: o.tm_max = atof(a); break;
		case STRAND: o.primer_strand = atof(a); break;
		case SALT: o.salt = atof(a); break;
		case HAIRPIN: o.max_hairpin = atof(a); break;
		case DIMER: o.max_dimer = atof(a); break;
		case TARGET_NORMALIZE: o.normalize_target = true; break;
		case BACKGROUND_NORMALIZE: o.normalize_background = true; break;
		case THREAD: o.threads = (unsigned)abs(atoi(a)); break;
		case TARGET_SIZE_MIN: o.target_size_min = atoi(a); break;
		case TARGET_SIZE_MAX: o.target_size_max = atoi(a); break;
		case BACKGROUND_SIZE_MIN: o.background_size_min = atoi(a); break;
		case BACKGROUND_SIZE_MAX: o.background_size_max = atoi(a); break;
		case OPT5: o.optimize_5 = true; break;
		case NO_OPT5: o.optimize_5 = false; break;
		case OPT3: o.optimize_3 = true; break;
		case NO_OPT3: o.optimize_3 = false; break;
		case JSON_FILE: case JSON_ROOT: o.json_config = true; break;
		case TARGET_PREFIX: o.target_prefix = a; break;
		case BACKGROUND_PREFIX: o.background_prefix = a; break;
		case INPUT_PREFIX: o.input_prefix = a; break;
		case OUT_TEXT: o.json = false; break;
		case OUT_JSON: o.json = true; break;
		default: fprintf(stderr, "\"%c\" is not a valid option!\n", (char)c); return QUIT;
		}
	}
	if(print_usage){ usage(); return QUIT; }
	if(o.json_config){
		fprintf(stderr, "pcramp: the JSON configuration input (--json, --json.root) is not supported; give the options on the command line\n");
		return REFUSE;
	}
	if(o.target_files.empty() && o.target_dirs.empty()) return quit("Please specify one or more target filenames (-t) or directories (-T)");
	if(o.output.empty()) return quit("Please specify an output filename (-o)");
	if(o.degen == 0) return quit("Please specify a valid maximum degeneracy (-d)");
	if(o.primer_max > 32) return quit("The maximum primer length must be <= 32");
	if(o.primer_max < o.primer_min) return quit("The maximum primer length must be >= minimum primer length");
	if(o.tm_min > o.tm_max) return quit("The maximum primer melting temperature must be >= minimum primer melting temperature");
	if(o.target_amp_max < o.target_amp_min) return quit("The maximum target amplicon length must be >= minimum target amplicon length");
	if(o.background_amp_max < o.background_amp_min)
		return quit("The maximum background amplicon length must be >= minimum background amplicon length");
	if(o.target_size_max < o.target_size_min)
		return quit("The maximum target input sequence length must be >= minimum target input sequence length");
	if(o.background_size_max < o.background_size_min)
		return quit("The maximum background input sequence length must be >= minimum background input sequence length");
	if(o.pack_max_gc < o.pack_min_gc) return quit("The maximum packing GC content must be >= the minimum packing GC content");
	if(o.seed == 0) o.seed = (unsigned)time(nullptr);
	if(o.salt < 0.0f) return quit("Please specify a salt concentration > 0");
	if(o.primer_strand < 0.0f) return quit("Please specify a [primer strand] concentration > 0");
	make_set(o.target_files);
	make_set(o.background_files);
	for(auto *dirs : {&o.target_dirs, &o.background_dirs}){
		for(std::string &d : *dirs)
			while(!d.empty() && d.back() == '/') d.pop_back();
		make_set(*dirs);
	}
	if(o.target_prefix.empty()) o.target_prefix = o.input_prefix;
	if(o.background_prefix.empty()) o.background_prefix = o.input_prefix;
	for(const std::string &d : o.target_dirs){
		const std::string path = o.target_prefix.empty() ? d : o.target_prefix + '/' + d;
		if(!find_groups(path, o.target_groups)){ fprintf(stderr, "Invalid target path: %s\n", path.c_str()); return QUIT; }
	}
	for(const std::string &d : o.background_dirs){
		const std::string path = o.background_prefix.empty() ? d : o.background_prefix + '/' + d;
		if(!find_groups(path, o.background_groups)){ fprintf(stderr, "Invalid background path: %s\n", d.c_str()); return QUIT; }
	}
	for(auto *groups : {&o.target_groups, &o.background_groups})
		for(auto &g : *groups) std::sort(g.second.begin(), g.second.end());
	return RUN;
}

// ---- FASTA ingest

// Sequence::extract_weight (sequence.cpp:332-490): the first complete "[w=value]" tag of a defline gives its weight.  Restated as a
// scan: '[' opens a tag (more '[' and blanks may follow), then 'w' or 'W', blanks, '=', blanks, then the value characters
// (digits, sign, '.', 'e'), blanks, and ']' closes it.  Any other character abandons the tag; a '[' after the opening one starts
// a new tag.  The value handed to atof runs from its first character to its last one -- or, when the value is a single
// character, to the end of the defline (atof stops at the first character it cannot use either way).  No tag: weight 1.
float defline_weight(const std::string &d)
{
	auto blank = [](char c) { return c == ' ' || c == '\t'; };
	auto value_char = [](char c) { return (c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.' || c == 'e'; };
	const size_t n = d.size();
	for(size_t i = 0;i < n;){
		if(d[i] != '['){ ++i; continue; }
		size_t k = i + 1;
		while(k < n && (blank(d[k]) || d[k] == '[')) ++k;                      // after '[': blanks and more '['
		if(k >= n) break;
		if(d[k] != 'w' && d[k] != 'W'){ i = k + 1; continue; }
		++k;
		while(k < n && blank(d[k])) ++k;
		if(k >= n) break;
		if(d[k] == '['){ i = k; continue; }
		if(d[k] != '='){ i = k + 1; continue; }
		++k;
		while(k < n && blank(d[k])) ++k;
		if(k >= n) break;
		if(d[k] == '['){ i = k; continue; }
		if(!value_char(d[k])){ i = k + 1; continue; }
		const size_t first = k;
		size_t last = std::string::npos;                                      // a single-character value has no last one
		++k;
		while(k < n && value_char(d[k])) last = k++;
		while(k < n && blank(d[k])) ++k;
		if(k >= n) break;
		if(d[k] == ']') return (float)atof(d.substr(first, last == std::string::npos ? std::string::npos : last - first + 1).c_str());
		if(d[k] == '['){ i = k; continue; }
		i = k + 1;
	}
	return 1.0f;
}

bool ignored(const std::string &defline, const std::vector<std::string> &keys)
{
	if(keys.empty()) return false;
	const std::string d = lower(defline);
	for(const std::string &k : keys)
		if(d.find(k) != std::string::npos) return true;
	return false;
}

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

// byte -> class: 0..15 the 4-bit code of base_to_bits (base_table.h:31-76; A=1 C=2 G=4 T=8, IUPAC unions, '-' = EOS = 0),
// or one of the markers below
enum : uint8_t { C_SPACE = 16, C_DEFLINE, C_END, C_ILLEGAL };
struct ByteClasses {
	uint8_t c[256];
	ByteClasses()
	{
		memset(c, C_ILLEGAL, sizeof(c));
		const char *sym = "-ACMGRSVTWYHKDBN";
		for(int k = 0;k < 16;++k) c[(uint8_t)sym[k]] = c[(uint8_t)tolower(sym[k])] = (uint8_t)k;
		c['U'] = c['u'] = 8;
		c['I'] = c['i'] = c['X'] = c['x'] = 15;
		for(int s : {' ', '\t', '\n', '\v', '\f', '\r'}) c[s] = C_SPACE;        // isspace() in the C locale
		c['>'] = C_DEFLINE;
		c[0] = C_END;                                                          // gzgets hands back C strings
	}
};
const ByteClasses kClass;

// A growable byte array that does not clear what it grows into.
struct Bytes {
	std::unique_ptr<uint8_t[]> p;
	size_t n = 0, cap = 0;
	uint8_t *reserve_tail(size_t extra)
	{
		if(n + extra > cap){
			const size_t c = std::max(n + extra, cap * 2 + (1u << 20));
			std::unique_ptr<uint8_t[]> q(new uint8_t[c]);
			if(n) memcpy(q.get(), p.get(), n);
			p.swap(q);
			cap = c;
		}
		return p.get() + n;
	}
};

// One sequence set as pcr_load_sequences takes it, built one base code per byte and packed at the end.
struct SeqSet {
	Bytes codes;
	std::vector<uint64_t> start, len;
	std::vector<float> weight;
	std::vector<std::string> defline;
};

// The pieces gzgets(fin, buf, 2048) returns, read in large blocks: up to and including the next '\n', at most 2047 bytes.
class Chunks {
	static constexpr size_t kChunk = 2047, kBlock = 8u << 20;
	gzFile f_;
	std::unique_ptr<char[]> buf_{new char[kBlock]};
	size_t pos_ = 0, end_ = 0;
	bool eof_ = false;
public:
	explicit Chunks(const std::string &path) : f_(gzopen(path.c_str(), "r"))
	{
		if(!f_){
			fprintf(stderr, "Error opening: %s\n", path.c_str());
			throw Error("Unable to open fasta file");
		}
		gzbuffer(f_, 1u << 20);
	}
	~Chunks() { gzclose(f_); }
	bool next(const char *&p, size_t &n)
	{
		for(;;){
			const size_t avail = end_ - pos_, lim = std::min(avail, kChunk);
			const char *b = buf_.get() + pos_;
			if(const void *nl = memchr(b, '\n', lim)) n = (size_t)((const char *)nl - b) + 1;
			else if(lim == kChunk || (eof_ && avail)) n = lim;
			else if(eof_) return false;
			else{
				memmove(buf_.get(), b, avail);
				pos_ = 0;
				end_ = avail;
				const int got = gzread(f_, buf_.get() + end_, (unsigned)(kBlock - end_));
				if(got <= 0) eof_ = true;                                      // end of file or a read error: gzgets stops either way
				else end_ += (size_t)got;
				continue;
			}
			p = b;
			pos_ += n;
			return true;
		}
	}
};

struct Filter {
	size_t min_len, max_len;
	const std::vector<std::string> *ignore;
};

// parse_fasta / append_fasta_group (parse_fasta.cpp): the records of one file.  A piece holding '>' is a defline (cut at its
// first CR or LF); in any other piece every non-blank byte is one base.  A record is kept when its base count lies in
// [min_len, max_len] and its defline holds no ignore key; a defline that follows no bases replaces the one before.  Only kept
// records are checked for illegal bases.  `group` < 0: each kept record becomes a sequence of `S`; otherwise the kept records are
// appended to the open sequence that starts at code `group`, one EOS between two of them.  Returns the number of records kept.
size_t read_fasta(const std::string &path, const Filter &flt, SeqSet &S, int64_t group)
{
	Chunks in(path);
	std::string def;
	size_t kept = 0, mark = 0;
	bool bad = false;
	const uint8_t *cls = kClass.c;
	const char *p;
	size_t len;
	// the bases of the open record sit at [mark, S.codes.n); in group mode, when the group already holds bases, the EOS in
	// front of them at mark - 1 (removed again with a dropped record)
	bool padded = false;
	auto open = [&]() {
		padded = group >= 0 && S.codes.n > (uint64_t)group;
		if(padded){ *S.codes.reserve_tail(1) = 0; ++S.codes.n; }
		mark = S.codes.n;
		bad = false;
	};
	auto close = [&]() {
		const size_t n = S.codes.n - mark;
		if(n >= flt.min_len && n <= flt.max_len && !ignored(def, *flt.ignore)){
			if(bad){
				fprintf(stderr, "Illegal base in the record \"%s\" of %s\n", def.c_str(), path.c_str());
				throw Error("Illegal base");
			}
			if(group < 0){
				const float w = defline_weight(def);
				if(w < 0.0f) throw Error("Sequence::defline: Negative weights are not allowed!");
				S.start.push_back(mark);
				S.len.push_back(n);
				S.weight.push_back(w);
				S.defline.push_back(def);
			}
			++kept;
		}
		else S.codes.n = padded ? mark - 1 : mark;
	};
	open();
	while(in.next(p, len)){
		uint8_t *out = S.codes.reserve_tail(len), *o = out;
		bool chunk_bad = false, is_defline = false;
		for(size_t i = 0;i < len;++i){
			const uint8_t k = cls[(uint8_t)p[i]];
			if(k < 16) *o++ = k;
			else if(k == C_SPACE) continue;
			else if(k == C_ILLEGAL){ *o++ = 0; chunk_bad = true; }
			else if(k == C_END) break;
			else{ is_defline = true; break; }
		}
		if(!is_defline){
			S.codes.n += (size_t)(o - out);
			bad |= chunk_bad;
			continue;
		}
		if(S.codes.n > mark){                                                  // a defline after bases ends the record
			close();
			open();
		}
		size_t e = 0;
		while(e < len && p[e] != '\n' && p[e] != '\r' && p[e] != '\0') ++e;
		def.assign(p, e);
	}
	close();                                                                   // the last record: kept even when empty if min_len is 0
	return kept;
}

struct SetSpec {
	const std::vector<std::string> *files;
	const std::map<std::string, std::vector<std::string>> *groups;
	const std::string *prefix;
	Filter filter;
	bool normalize;
};

// main.cpp:253-344 (targets) / :346-436 (backgrounds): the -t / -b files in sorted order, each record a sequence (weights 1 / kept
// records of its file with --*.normalize), then the -T / -B groups in sorted order of their names, each one sequence.
void read_set(const SetSpec &s, SeqSet &S)
{
	for(const std::string &f : *s.files){
		const size_t first = S.len.size();
		const size_t kept = read_fasta(f, s.filter, S, -1);
		if(s.normalize && kept){
			const float w = (float)(1.0/kept);
			for(size_t i = first;i < S.len.size();++i) S.weight[i] = w;
		}
	}
	for(const auto &g : *s.groups){
		if(ignored(g.first, *s.filter.ignore)) continue;
		std::string name = g.first;                                            // the group name without the prefix and leading '/'
		if(name.compare(0, s.prefix->size(), *s.prefix) == 0){
			name.erase(0, s.prefix->size());
			name.erase(0, name.find_first_not_of('/') == std::string::npos ? name.size() : name.find_first_not_of('/'));
		}
		const float w = defline_weight(name);
		if(w < 0.0f) throw Error("Sequence::defline: Negative weights are not allowed!");
		const uint64_t start = S.codes.n;
		for(const std::string &f : g.second) read_fasta(f, s.filter, S, (int64_t)start);
		if(S.codes.n == start) continue;                                       // nothing kept: the group is dropped
		S.start.push_back(start);
		S.len.push_back(S.codes.n - start);
		S.weight.push_back(w);
		S.defline.push_back(name);
	}
}

// 4-bit codes, two bases per byte, high nibble first; each sequence starts on a byte
void pack(const SeqSet &S, std::vector<uint8_t> &packed, std::vector<uint64_t> &offsets)
{
	offsets.resize(S.len.size());
	uint64_t total = 0;
	for(size_t i = 0;i < S.len.size();++i){ offsets[i] = total; total += (S.len[i] + 1)/2; }
	packed.assign(std::max<uint64_t>(total, 1), 0);                              // never a null pointer, even for zero-length sequences only
	for(size_t i = 0;i < S.len.size();++i){
		const uint8_t *c = S.codes.p.get() + S.start[i];
		uint8_t *o = packed.data() + offsets[i];
		const uint64_t n = S.len[i];
		for(uint64_t j = 0;j + 1 < n;j += 2) *o++ = (uint8_t)(c[j] << 4 | c[j + 1]);
		if(n & 1) *o = (uint8_t)(c[n - 1] << 4);
	}
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

int main(int argc, char **argv)
{
	const auto t0 = std::chrono::steady_clock::now();
	Options opt;
	const Status st = load_options(argc, argv, opt);
	if(st == QUIT) return EXIT_SUCCESS;
	if(st == REFUSE) return EXIT_FAILURE;

	// the output file is opened and its first lines written before any input is read (main.cpp:125-163)
	FILE *out = fopen(opt.output.c_str(), "wb");
	if(!out){
		fprintf(stderr, "Caught the error Unable to open output file for writing: %s\n", opt.output.c_str());
		return EXIT_FAILURE;
	}
	const int64_t np = pcr_format_preamble(opt.json, argc, argv, opt.seed, nullptr, 0);
	std::string preamble((size_t)std::max<int64_t>(np, 0) + 1, '\0');
	if(np < 0 || pcr_format_preamble(opt.json, argc, argv, opt.seed, &preamble[0], preamble.size()) != np){
		fprintf(stderr, "Caught the error %s\n", pcr_last_error());
		fclose(out);
		return EXIT_FAILURE;
	}
	preamble.resize((size_t)np);
	fwrite(preamble.data(), 1, preamble.size(), out);
	fflush(out);

	SeqSet T, B;
	try{
		// per-record length limits: max(amplicon.min, size.min) .. size.max (main.cpp:262-265), as size_t
		const SetSpec ts{&opt.target_files, &opt.target_groups, &opt.target_prefix,
			{(size_t)std::max(opt.target_amp_min, opt.target_size_min), (size_t)opt.target_size_max, &opt.target_ignore}, opt.normalize_target};
		const SetSpec bs{&opt.background_files, &opt.background_groups, &opt.background_prefix,
			{(size_t)std::max(opt.background_amp_min, opt.background_size_min), (size_t)opt.background_size_max, &opt.background_ignore},
			opt.normalize_background};
		read_set(ts, T);
		read_set(bs, B);
	}
	catch(const std::exception &e){
		fprintf(stderr, "Caught the error %s\n", e.what());
		fclose(out);
		return EXIT_FAILURE;
	}
	std::vector<uint8_t> tp, bp;
	std::vector<uint64_t> toff, boff;
	pack(T, tp, toff);
	pack(B, bp, boff);
	uint64_t bases = 0;
	for(uint64_t l : T.len) bases += l;
	for(uint64_t l : B.len) bases += l;
	T.codes = Bytes();
	B.codes = Bytes();
	if(opt.verbosity != SILENT)
		fprintf(stderr, "Read %zu target and %zu background sequences (%llu bases) in %.3f s\n", T.len.size(), B.len.size(),
		        (unsigned long long)bases, seconds_since(t0));

	auto fail = [&](const char *what) {
		fprintf(stderr, "Caught the error %s: %s\n", what, pcr_last_error());
		fclose(out);
		return EXIT_FAILURE;
	};
	if(T.len.empty()){
		// the reference trips an assertion in its sampler (PCR::random_assay) when no target is left
		fprintf(stderr, "Caught the error no target sequence is left after the input filters\n");
		fclose(out);
		return EXIT_FAILURE;
	}
	pcr_params params{opt.pack_max_degen, opt.pack_min_gc, opt.pack_max_gc};
	pcr_ctx *ctx = pcr_create(0, nullptr, &params);
	if(!ctx) return fail("pcr_create");
	if(pcr_load_sequences(ctx, PCR_SET_TARGET, tp.data(), toff.data(), T.len.data(), T.weight.data(), (uint32_t)T.len.size()) != PCR_OK ||
	   (!B.len.empty() &&
	    pcr_load_sequences(ctx, PCR_SET_BACKGROUND, bp.data(), boff.data(), B.len.data(), B.weight.data(), (uint32_t)B.len.size()) != PCR_OK)){
		pcr_destroy(ctx);
		return fail("pcr_load_sequences");
	}
	std::vector<const char *> tdef, bdef;
	for(const std::string &d : T.defline) tdef.push_back(d.c_str());
	for(const std::string &d : B.defline) bdef.push_back(d.c_str());
	const pcr_output o{opt.json, 1, (uint32_t)T.len.size(), (uint32_t)B.len.size(), tdef.data(), bdef.data(), T.len.data(), B.len.data()};
	pcr_design_args a{};
	a.num_assay = opt.num_assay;
	a.num_trial = opt.num_trial;
	a.seed = opt.seed;
	a.top_down_search = opt.top_down;
	a.optimize_5 = opt.optimize_5;
	a.optimize_3 = opt.optimize_3;
	a.target_threshold = opt.target_threshold;
	a.target_search_multiplier = opt.target_search;
	a.background_threshold = opt.background_threshold;
	a.background_search_multiplier = opt.background_search;
	a.min_target_cover = opt.min_target_cover;
	a.max_background_cover = opt.max_background_cover;
	a.target_amp_min = opt.target_amp_min;
	a.target_amp_max = opt.target_amp_max;
	a.background_amp_min = opt.background_amp_min;
	a.background_amp_max = opt.background_amp_max;
	a.primer_min = opt.primer_min;
	a.primer_max = opt.primer_max;
	a.max_degen = (double)opt.degen;
	a.thermo = pcr_thermo_args{opt.salt, opt.primer_strand, opt.tm_min, opt.tm_max, opt.max_hairpin, opt.max_dimer};
	a.use_taq_mama = opt.taq_mama;
	a.use_multiplex = 1;
	if(opt.verbosity != SILENT) fprintf(stderr, "Sequences loaded on the GPU; the design starts at %.3f s\n", seconds_since(t0));
	const int rc = pcr_design(ctx, &a, &o, argc, argv, nullptr, 0, nullptr);
	uint64_t n = 0;
	const char *text = pcr_design_output(ctx, &n);
	// the design output begins with the lines already written
	if(text && n >= preamble.size() && memcmp(text, preamble.data(), preamble.size()) == 0)
		fwrite(text + preamble.size(), 1, n - preamble.size(), out);
	else if(rc == PCR_OK){
		pcr_destroy(ctx);
		fclose(out);
		fprintf(stderr, "Caught the error the design output does not begin with the command line written\n");
		return EXIT_FAILURE;
	}
	if(rc != PCR_OK){
		const int r = fail("pcr_design");
		pcr_destroy(ctx);
		return r;
	}
	pcr_destroy(ctx);
	if(fclose(out) != 0){
		fprintf(stderr, "Caught the error Unable to write the output file\n");
		return EXIT_FAILURE;
	}
	return EXIT_SUCCESS;
}

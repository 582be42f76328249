"""Writes tests/golden/cli.json: whole runs of the reference PROGRAM (oracle/_ref/pcramp, made by __graft_entry__.build()) on
FASTA inputs laid out on disk -- what `pcramp` reads before its design loop starts (main.cpp:253-436, parse_fasta.cpp,
Sequence::defline, Options::load and find_groups of options.cpp).  A script, not a test: run it where the reference binary and
the MPICH it was linked against exist.

Every case is a recipe (tests/cli_cases.py: an input seed and pool spec for tests/testdata.py, the files with their deflines,
line width, line ends, compression and special records) and a command line.  It runs in a fresh directory at one thread with a
fixed seed, twice, and is kept only if both runs agree; the file records the exit status, whether out.txt exists and its bytes.
`stage` says how far the reference got: "quit" (opt.quit: no output file, EXIT_SUCCESS), "ingest" (thrown while reading the
inputs: only the version / command line / seed lines) or "design".  tests/test_cli_host.py replays the first two without a
GPU, tests/test_gpu_cli.py the rest through pcramp_amd/bin/pcramp.

    python tests/make_golden_cli.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from cli_cases import materialize  # noqa: E402

EXE = os.path.join(ROOT, "oracle", "_ref", "pcramp")
OUT = os.path.join(HERE, "golden", "cli.json")
REPEATS = 2
POOL = dict(n_fam=3, per=4, L=500, div=0.03)         # sequences 0-3, 4-7 (507 bases), 8-11 (514 bases): three families


def fa(path, records, **kw):
    return dict(path=path, records=records, **kw)


def R(d, s):
    return {"def": d, "seq": s}


def run_args(seed, count=2, trial=20):
    return ["--thread", "1", "--count", str(count), "--trial", str(trial), "--seed", str(seed)]


def targets(n=8, names=None, first=0):
    return [R(">t%d" % i if names is None else names[i - first], i) for i in range(first, first + n)]


def backgrounds(idx=(8, 9)):
    return [R(">bg%d" % i, {"of": i, "sub": [[40 + 7 * k, "A"] for k in range(30)]}) for i in idx]


def cases():
    c = []

    def add(name, files, argv, seed=7, dirs=()):
        c.append({"name": name, "input_seed": seed, "pool": POOL, "files": files, "dirs": list(dirs), "argv": ["pcramp"] + argv})

    bg = fa("b.fa", backgrounds())
    # ---- weights: the [w=x] tag in its spellings, zero, malformed
    add("weights", [fa("t.fa", [R(">t0 [w=2]", 0), R(">t1 [ w = 0.5 ]", 1), R(">t2 [[w=3]", 2), R(">t3 [W=1.5e0] x", 3),
                                R(">t4 [w=0]", 4), R(">t5 [w=abc]", 5), R(">t6\t[w\t=\t4 ]", 6), R(">t7 [x=5] [w=0.25]", 7)]), bg],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt"] + run_args(11))
    add("weights_more", [fa("t.fa", [R(">a [w=1.2.3]", 0), R(">b [w=+2]", 1), R(">c [w=2", 2), R(">d w=3]", 3),
                                     R(">e [w= 7]", 4), R(">f [w =.5]", 5), R(">g [w=[w=2]", 6), R(">h [w=3][w=9]", 7)]),
                         fa("b.fa", [R(">bg [w=0]", {"of": 8, "sub": [[40 + 7 * k, "A"] for k in range(30)]}), R(">bg2 [w=2.5]", 9)])],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt", "--background.cover", "1"] + run_args(12, count=3))
    add("weights_zero_all", [fa("t.fa", [R(">z%d [w=0]" % i, i) for i in range(4)] + [R(">one", 4)])],
        ["-t", "t.fa", "-o", "out.txt"] + run_args(13))
    add("negative_filtered", [fa("t.fa", targets(4) + [R(">short [w=-1]", {"of": 5, "to": 60})])],
        ["-t", "t.fa", "-o", "out.txt"] + run_args(14))
    # ---- per-file normalisation
    add("normalize", [fa("a.fa", [R(">a0", 0), R(">a1 [w=5]", 1), R(">a2", 4)]), fa("b.fa", [R(">b0", 5)]),
                      fa("c.fa", backgrounds((8, 9))), fa("d.fa", backgrounds((10,)))],
        ["-t", "a.fa", "-t", "b.fa", "--target.normalize", "-b", "c.fa", "-b", "d.fa", "--background.normalize", "-o", "out.txt"]
        + run_args(15, count=3))
    add("normalize_targets_only", [fa("a.fa", [R(">a0", 0), R(">a1", 1), R(">a2", 2), R(">a3", 3)]), fa("b.fa", [R(">b0 [w=3]", 4)]), dict(bg, path="z.fa")],
        ["-t", "a.fa", "-t", "b.fa", "--target.normalize", "-b", "z.fa", "-o", "out.txt"] + run_args(16))
    # ---- ignore keywords
    add("ignore", [fa("t.fa", [R(">keep_1", 0), R(">SKIPME 2", 1), R(">x skipme", 4), R(">y", 5), R(">z SkIpMe", 6)]),
                   fa("b.fa", [R(">bg PLASMID", 8), R(">bg ok", {"of": 9, "sub": [[40 + 7 * k, "A"] for k in range(30)]})])],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt", "--target.ignore", "skipme", "--background.ignore", "Plasmid",
         "--background.ignore", "nothing"] + run_args(17))
    # ---- size filters and the max(amplicon.min, size.min) rule
    add("size", [fa("t.fa", [R(">s75", {"of": 0, "to": 75}), R(">s120", {"of": 1, "to": 120}), R(">s300", {"of": 2, "to": 300}),
                             R(">s500", 3), R(">s507", 4), R(">s505", {"of": 5, "to": 505})]),
                 fa("b.fa", [R(">b90", {"of": 8, "to": 90}), R(">b200", {"of": 9, "to": 200}), R(">b500", {"of": 10, "to": 500})])],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt", "--target.size.min", "50", "--target.size.max", "505",
         "--background.size.min", "100", "--background.size.max", "450"] + run_args(18))
    add("size_amplicon_min", [fa("t.fa", [R(">s120", {"of": 0, "to": 120}), R(">s160", {"of": 1, "to": 160}), R(">s500", 2), R(">s501", 3)])],
        ["-t", "t.fa", "-o", "out.txt", "--target.amplicon.min", "150", "--target.size.min", "100",
         "--target.amplicon.max", "250"] + run_args(19))
    # ---- several -t files, out of order and twice
    add("file_order", [fa("c.fa", [R(">c0", 0), R(">c1", 1)]), fa("a.fa", [R(">a0", 4), R(">a1", 5)]), fa("b.fa", [R(">b0", 2)]), dict(bg, path="z.fa")],
        ["-t", "c.fa", "-t", "a.fa", "-t", "b.fa", "-t", "a.fa", "-b", "z.fa", "-b", "z.fa", "-o", "out.txt"] + run_args(20))
    # ---- compression and extensions
    add("gzip", [fa("t.fa.gz", [R(">g0", 0), R(">g1", 1)], width=70), fa("u.fasta", [R(">u0", 4), R(">u1", 5)]),
                 fa("b.fna.gz", backgrounds(), width=60), fa("v.fna", [R(">v0", 2)])],
        ["-t", "t.fa.gz", "-t", "u.fasta", "-t", "v.fna", "-b", "b.fna.gz", "-o", "out.txt"] + run_args(21))
    # ---- text quirks: CR LF, blank lines, case, IUPAC / U / X / I, a defline over 2047 bytes, sequence before the first
    # defline, an empty record, a '>' inside a line
    long_def = ">long " + "ACGT" * 600
    add("format", [fa("t.fa", [R(None, 0), R(">lower", {"of": 1, "lower": 1}),
                               R(">iupac", {"of": 2, "sub": [[10, "R"], [50, "u"], [90, "X"], [130, "n"], [170, "I"], [210, "y"]]}),
                               R(">empty", ""), R(">after_empty", 3), R(long_def, {"of": 4, "to": 300}), R(">plain", 5)],
                      crlf=1, blank=1, width=60)],
        ["-t", "t.fa", "-o", "out.txt"] + run_args(22))
    add("format_inline_gt", [fa("t.fa", [R(">t0", 0), {"raw": "ACGTACGT>inline defline\n"}, R(None, 1), R(">t2", {"of": 2, "sub": [[100, "-"]]}),
                                         R(">t3", 3)], width=80, tail=">dangling\n")],
        ["-t", "t.fa", "-o", "out.txt"] + run_args(23))
    add("illegal_filtered", [fa("t.fa", targets(4) + [R(">bad but short", "ACGTZZACGT"), R(">bad ignored", {"of": 5, "sub": [[9, "Z"]]})])],
        ["-t", "t.fa", "-o", "out.txt", "--target.ignore", "ignored"] + run_args(24))
    add("empty_background", [fa("t.fa", targets(6)), fa("e.fa", [])], ["-t", "t.fa", "-b", "e.fa", "-o", "out.txt"] + run_args(25))
    # ---- groups: -T / -B trees of single-file groups, directory-name weights, a file named on its own, the prefixes
    tree = [fa("T/top.fa", [R(">top0", 0), R(">top1", 1)]), fa("T/g1/a.fa", [R(">a0", 4), R(">a1", 5), R(">a2", 6)]),
            fa("T/g2[w=2]/x.fna.gz", [R(">x0", 2), R(">x1", 3)], width=50), fa("T/g3/sub/y.fasta", [R(">y0", 7)]),
            fa("T/notes/readme.txt", [R(">not fasta", 0)]),
            fa("B/h1/z.fa", backgrounds((8, 9)), tail=">dangling\n"), fa("B/h2/w.fa", backgrounds((10,))),
            fa("t.fa", [R(">single", {"of": 1, "to": 400})]), fa("S/solo.fa", [R(">solo0", {"of": 6, "from": 20}), R(">solo1", 7)])]
    add("tree", tree, ["-t", "t.fa", "-T", "T", "-B", "B/", "-o", "out.txt"] + run_args(26, count=3), dirs=["T/empty"])
    add("tree_file_group", tree, ["-T", "S/solo.fa", "-T", "T/g1", "-o", "out.txt"] + run_args(27))
    pre = [dict(f, path="pre/" + f["path"]) for f in tree]
    add("prefix_T_B", pre, ["-T", "T", "--T.prefix", "pre", "-B", "B", "--B.prefix", "pre/", "-o", "out.txt"] + run_args(28), dirs=["pre/T/empty"])
    add("prefix_input", pre, ["-T", "T/g1", "-T", "T/g2[w=2]", "-B", "B", "--input.prefix", "pre", "-o", "out.txt"] + run_args(29))
    add("prefix_target_long", pre, ["-T", "T", "--target.prefix", "pre", "--input.prefix", "pre", "-o", "out.txt"] + run_args(30))
    add("tree_filters", tree, ["-T", "T", "-B", "B", "--target.ignore", "g3", "--target.ignore", "a1", "--target.size.max", "505",
                               "--background.ignore", "h2", "-o", "out.txt"] + run_args(31))
    add("tree_json", tree, ["-T", "T", "-B", "B", "-t", "t.fa", "--o.json", "-o", "out.txt"] + run_args(32, count=3))
    # ---- the pack filters
    add("pack", [fa("t.fa", [R(">p%d" % i, {"of": i, "sub": [[17 * k + i, "RYKMSWN"[k % 7]] for k in range(25)]}) for i in range(6)]), bg],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt", "--pack.degen.max", "4", "--pack.gc.min", "0.3", "--pack.gc.max", "0.7", "-d", "4"]
        + run_args(33))
    add("pack_json", [fa("t.fa", targets(6)), bg],
        ["-t", "t.fa", "-b", "b.fa", "--o.json", "-o", "out.txt", "--pack.gc.max", "0.55", "--pack.degen.max", "1"] + run_args(34))
    # ---- getopt: abbreviations, "=value", a stray argument moved behind the switches, --o.text after --o.json, the no- switches
    add("getopt", [fa("t.fa", targets(6)), bg],
        ["-t", "t.fa", "stray", "-o", "out.txt", "--see=35", "--cou", "2", "--tri=20", "--thread", "1", "--o.json", "--o.text",
         "--optimize.5", "--no-optimize.5", "--optimize.3", "-b", "b.fa", "--target.weight", "2", "--background.weight", "0.5",
         "-v", "SILENT", "--primer.tm.min", "52", "--salt", "0.06"])
    # ---- quits: usage, unknown switch, missing -o / -t, bad paths, values out of range (no output file, exit 0)
    t_only = [fa("t.fa", targets(4))]
    for name, argv in [("help", ["-t", "t.fa", "-o", "out.txt", "-h"]), ("help_question", ["-?", "-t", "t.fa", "-o", "out.txt"]),
                       ("unknown_switch", ["-t", "t.fa", "-o", "out.txt", "--bogus"]), ("no_arguments", []),
                       ("missing_value", ["-t", "t.fa", "-o", "out.txt", "--seed"]), ("no_output", ["-t", "t.fa"]),
                       ("no_target", ["-o", "out.txt"]), ("bad_T_path", ["-T", "missing", "-o", "out.txt"]),
                       ("bad_B_path", ["-t", "t.fa", "-B", "missing", "-o", "out.txt"]),
                       ("T_not_fasta", ["-T", "T/notes/readme.txt", "-o", "out.txt"]),
                       ("threshold_range", ["-t", "t.fa", "-o", "out.txt", "--target.threshold", "1.5"]),
                       ("bg_threshold_range", ["-t", "t.fa", "-o", "out.txt", "--background.threshold", "-0.1"]),
                       ("verbosity", ["-t", "t.fa", "-o", "out.txt", "-v", "loud"]), ("trial_zero", ["-t", "t.fa", "-o", "out.txt", "--trial", "0"]),
                       ("primer_max", ["-t", "t.fa", "-o", "out.txt", "--primer.size.max", "33"]),
                       ("primer_order", ["-t", "t.fa", "-o", "out.txt", "--primer.size.min", "26"]),
                       ("gc_order", ["-t", "t.fa", "-o", "out.txt", "--pack.gc.min", "0.7", "--pack.gc.max", "0.3"]),
                       ("size_order", ["-t", "t.fa", "-o", "out.txt", "--target.size.min", "600", "--target.size.max", "500"]),
                       ("degen_zero", ["-t", "t.fa", "-o", "out.txt", "-d", "0"]), ("count_zero", ["-t", "t.fa", "-o", "out.txt", "--count", "0"]),
                       ("search_range", ["-t", "t.fa", "-o", "out.txt", "--target.search", "0"]),
                       ("target_weight_range", ["-t", "t.fa", "-o", "out.txt", "--target.weight", "0.5"]),
                       ("amplicon_order", ["-t", "t.fa", "-o", "out.txt", "--target.amplicon.min", "300"]),
                       ("salt_negative", ["-t", "t.fa", "-o", "out.txt", "--salt", "-1"])]:
        add("quit_" + name, t_only + [tree[4]], (run_args(40) + argv) if argv else [])
    # ---- throws while reading: only the first lines are written, exit 1
    add("throw_missing_file", t_only, ["-t", "t.fa", "-t", "nothere.fa", "-o", "out.txt"] + run_args(41))
    add("throw_illegal_base", [fa("t.fa", targets(3) + [R(">bad", {"of": 4, "sub": [[77, "Z"]]})])], ["-t", "t.fa", "-o", "out.txt"] + run_args(42))
    add("throw_illegal_json", [fa("t.fa", [R(">bad", {"of": 4, "sub": [[7, "J"]]})])], ["-t", "t.fa", "-o", "out.txt", "--o.json"] + run_args(43))
    add("throw_illegal_background", t_only + [fa("b.fa", [R(">bg", {"of": 8, "sub": [[3, "."]]})])],
        ["-t", "t.fa", "-b", "b.fa", "-o", "out.txt"] + run_args(44))
    add("throw_negative_weight", [fa("t.fa", targets(3) + [R(">neg [w=-0.5]", 4)])], ["-t", "t.fa", "-o", "out.txt"] + run_args(45))
    add("throw_negative_group", [fa("T/g[w=-2]/a.fa", targets(3))], ["-T", "T", "-o", "out.txt"] + run_args(46))
    add("throw_illegal_in_group", [fa("T/g/a.fa", targets(2) + [R(">bad", {"of": 4, "sub": [[7, "*"]]})])], ["-T", "T", "-o", "out.txt"] + run_args(47))
    add("throw_no_output_dir", t_only, ["-t", "t.fa", "-o", "nodir/out.txt"] + run_args(48))
    return c


def run_once(case, env):
    with tempfile.TemporaryDirectory() as tmp:
        materialize(case, tmp)
        pr = subprocess.run(case["argv"], executable=EXE, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        out_path = os.path.join(tmp, "out.txt")
        exists = os.path.exists(out_path)
        out = open(out_path, "rb").read().decode("latin-1") if exists else None
    return pr.returncode, exists, out, pr.stderr.decode("latin-1")[-200:]


def stage(status, exists, out):
    if status == 0 and not exists:
        return "quit"
    if status != 0 and (out is None or "sequence summary" not in out):
        return "ingest"
    return "design"


def main():
    if not os.path.exists(EXE):
        sys.exit("make_golden_cli: needs %s (build())" % EXE)
    libdir = tempfile.mkdtemp()
    try:
        for so in ("libmpi.so.12", "libgfortran.so.4", "libquadmath.so.0"):   # not the whole conda lib dir: its libstdc++ is older
            os.symlink(os.path.join("/opt/conda/lib", so), os.path.join(libdir, so))
        env = dict(os.environ, LD_LIBRARY_PATH=libdir, OMP_NUM_THREADS="1")
        runs, dropped = [], []
        for case in cases():
            first = run_once(case, env)
            if any(run_once(case, env)[:3] != first[:3] for _ in range(REPEATS - 1)):
                dropped.append(case["name"])
                print("dropped:", case["name"])
                continue
            status, exists, out, tail = first
            if status < 0:
                dropped.append(case["name"])
                print("dropped (the reference died by signal %d): %s %s" % (-status, case["name"], tail))
                continue
            st = stage(status, exists, out)
            runs.append(dict(case, status=status, exists=int(exists), output=out, stage=st))
            print("%-28s %-6s status %d%s" % (case["name"], st, status,
                                              "" if out is None else ", %d bytes, %d assays" % (len(out), out.count("ASSAY.") + out.count('"forward primer"'))))
    finally:
        shutil.rmtree(libdir)
    doc = {"note": "the reference program at one thread on FASTA trees rebuilt by tests/cli_cases.py; every case ran %d times and is "
                   "kept only if all runs agree (tests/make_golden_cli.py)" % REPEATS, "dropped": dropped, "runs": runs}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("%d runs, %d dropped -> %s (%d bytes)" % (len(runs), len(dropped), OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()

"""The input trees of tests/golden/cli.json, rebuilt from their recipes (tests/make_golden_cli.py writes them, tests/test_cli_host.py
and tests/test_gpu_cli.py replay them).

A case holds an input seed and a `pool` spec: sequence families drawn with tests/testdata.py as tests/golden/program.json's inputs
are.  Its `files` say where each FASTA file goes and how it is written:
    path     relative to the case directory; a name ending in .gz is gzip-compressed
    records  [{"def": defline or null (sequence text with no defline), "seq": <seq>}]; <seq> is an index into the pool, a
             literal string, or {"of": index, "from": a, "to": b, "lower": 0/1, "sub": [[position, character], ...]}
    width    bases per line (0 = one line per record)
    crlf     1 = CR LF line ends
    blank    1 = an empty line after every record
    head / tail   raw text written before the first / after the last record
`dirs` lists directories that must exist even when empty.  A record of {"raw": text} is written as it stands."""
import gzip
import os
import random

from make_golden_mpi import inputs as _program_run_inputs
from testdata import mutate, rand_seq


def pool(spec, seed):
    r = random.Random(seed)
    roots = [rand_seq(r, spec["L"] + 7 * k) for k in range(spec["n_fam"])]
    return [mutate(r, roots[k], spec["div"]) for k in range(spec["n_fam"]) for _ in range(spec["per"])]


def seq_text(s, seqs):
    if isinstance(s, int):
        return seqs[s]
    if isinstance(s, str):
        return s
    t = seqs[s["of"]][s.get("from", 0):s.get("to", None)]
    if s.get("sub"):
        t = list(t)
        for pos, ch in s["sub"]:
            t[pos] = ch
        t = "".join(t)
    return t.lower() if s.get("lower") else t


def file_bytes(f, seqs):
    eol = "\r\n" if f.get("crlf") else "\n"
    width = f.get("width", 0)
    out = [f.get("head", "")]
    for rec in f["records"]:
        if "raw" in rec:
            out.append(rec["raw"])
            continue
        if rec.get("def") is not None:
            out.append(rec["def"] + eol)
        t = seq_text(rec["seq"], seqs)
        if width:
            out.extend(t[i:i + width] + eol for i in range(0, len(t), width))
        elif t:
            out.append(t + eol)
        if f.get("blank"):
            out.append(eol)
    out.append(f.get("tail", ""))
    data = "".join(out).encode("latin-1")
    return gzip.compress(data, mtime=0) if f["path"].endswith(".gz") else data


def materialize(case, root):
    """Write the case's input tree under `root` (an existing, empty directory)."""
    seqs = pool(case["pool"], case["input_seed"]) if case.get("pool") else []
    for d in case.get("dirs", []):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for f in case.get("files", []):
        p = os.path.join(root, f["path"])
        os.makedirs(os.path.dirname(p) or root, exist_ok=True)
        with open(p, "wb") as fh:
            fh.write(file_bytes(f, seqs))


def program_inputs(run):
    """(targets, backgrounds) as [(defline, text)] of a tests/golden/program.json run (oracle/make_golden.py::program_golden)."""
    return _program_run_inputs(run["spec"], run["input_seed"])


# the input specs of oracle/make_golden.py::writers_golden, by run index of tests/golden/writers.json
WRITERS_SPECS = [dict(n_fam=3, per=4, L=600, n_bg=2), dict(n_fam=3, per=4, L=600, n_bg=2), dict(n_fam=1, per=4, L=500, n_bg=0),
                 dict(n_fam=1, per=4, L=500, n_bg=0), dict(n_fam=2, per=3, L=451, n_bg=3), dict(n_fam=2, per=3, L=451, n_bg=3)]


def writers_inputs(ri):
    sp = WRITERS_SPECS[ri]
    r2 = random.Random(6000 + ri // 2)
    roots = [rand_seq(r2, sp["L"] + 7 * k) for k in range(sp["n_fam"])]
    targets = [(">target_%d family %d" % (k * sp["per"] + j, k), mutate(r2, roots[k], 0.03))
               for k in range(sp["n_fam"]) for j in range(sp["per"])]
    bgs = [(">bg_%d" % i, mutate(r2, roots[i % len(roots)], 0.12)) for i in range(sp["n_bg"])]
    return targets, bgs


def write_program_inputs(root, targets, bgs):
    """t.fa / b.fa as the reference's golden runs read them: one line per defline and per sequence."""
    with open(os.path.join(root, "t.fa"), "w") as f:
        f.write("".join("%s\n%s\n" % (d, q) for d, q in targets))
    if bgs:
        with open(os.path.join(root, "b.fa"), "w") as f:
            f.write("".join("%s\n%s\n" % (d, q) for d, q in bgs))

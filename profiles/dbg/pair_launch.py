"""The paired launch on the GPU's clock (profiles/pair_launch.md): two C2 target sets on two handles of one stream, the
same two passes N times launched alone (PCRAMP_PAIR=0: k_seed3, k_post twice each) and N times as a pair
(PCRAMP_PAIR=force: k_seed3_pair, k_post_pair once each).  Run it under the profiler, the interpreter right behind `--`:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/dbg/pair_launch.py 300
    python profiles/dbg/pair_launch.py --stats OUT          # medians of the four kernels out of the trace
    python profiles/dbg/pair_launch.py --timeline OUT       # the same out of a trace of bench.py, with the share of paired passes

Every pair of passes is synchronised before the next is queued, so that what the trace shows is the kernels and not a
backlog; the bitsets of the two modes are compared at the end."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def stats(out_dir):
    import numpy as np
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by = {}
    for r in rows:
        name = r["Kernel_Name"]
        for k in ("k_seed3_pair", "k_post_pair", "k_seed3", "k_post<8>", "k_post"):
            if k in name:
                by.setdefault(k.replace("<8>", ""), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
                break
    for k in ("k_seed3", "k_post", "k_seed3_pair", "k_post_pair"):
        v = np.array(by.get(k, [0.0]))
        print("%-13s n %5d  median %6.2f  p10 %6.2f  p90 %6.2f us" % (k, len(v), np.median(v), np.percentile(v, 10), np.percentile(v, 90)))
    m = {k: float(np.median(by[k])) for k in by}
    if len(m) >= 4:
        single, pair = 2 * m["k_seed3"] + 2 * m["k_post"], m["k_seed3_pair"] + m["k_post_pair"]
        print("two single scans + two single tails %.2f us, paired scan + paired tail %.2f us: ratio %.2f" % (single, pair, pair / single))


def timeline(out_dir):
    """A trace of bench.py: the scans and tails, the share of passes that paired, the period per pass."""
    import numpy as np
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    by, starts = {}, []
    for r in rows:
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        for k in ("k_seed3_pair", "k_post_pair", "k_seed3", "k_post<8>"):
            if k in name:
                by.setdefault(k, []).append((t1 - t0) / 1000.0)
                if k.startswith("k_seed3"):
                    starts.append((t0, 2 if k == "k_seed3_pair" else 1))
                break
    for k, v in sorted(by.items()):
        v = np.array(v)
        print("%-13s n %6d  median %6.2f  p10 %6.2f  p90 %6.2f us" % (k, len(v), np.median(v), np.percentile(v, 10), np.percentile(v, 90)))
    starts.sort()
    n_pass = sum(w for _, w in starts)
    n_pair = sum(w for _, w in starts if w == 2)
    # the period per pass over windows of 64 consecutive scan launches (the loop's pauses -- warm-up, drains -- fall out of the median)
    per = []
    for i in range(0, len(starts) - 64, 64):
        per.append((starts[i + 64][0] - starts[i][0]) / 1000.0 / sum(w for _, w in starts[i:i + 64]))
    per = np.array(per if per else [0.0])
    print("passes %d, paired %d (%.1f %%); period per pass: median %.2f  p10 %.2f  p90 %.2f us" % (n_pass, n_pair, 100.0 * n_pair / max(n_pass, 1),
          np.median(per), np.percentile(per, 10), np.percentile(per, 90)))


def main(n):
    import numpy as np
    import torch
    from pcramp_amd import api, synth, words as W

    thr_t = 1.0
    thr = float(np.float32(thr_t) * np.float32(0.9))
    sets = [synth.GlobalSet("C2", 1, seed_base=j) for j in range(2)]
    pa = W.pairs_array(sets[0].pairs())
    got = {}
    for mode in ("0", "force"):
        os.environ["PCRAMP_PAIR"] = mode
        st = torch.cuda.Stream()
        hs = []
        for gs in sets:
            s = api.Screener(0, stream=st.cuda_stream)
            s.load_sequences(*gs.members(0, gs.T))
            hs.append(s)
        words = int(hs[0].bitset_words())
        with torch.cuda.stream(st):
            out = torch.zeros((2, 2, len(pa), words), dtype=torch.int64, device="cuda:0")
        st.synchronize()
        calls = [h.screen_call(pa, thr, out[j, 0].data_ptr(), out[j, 1].data_ptr(), thr_t, thr_t, 80, 200, False, 18, False, False) for j, h in enumerate(hs)]
        for c in calls:                               # (the first pass over a set builds its index, inline)
            c()
        for h in hs:
            h.synchronize()
        for _ in range(n):
            calls[0]()
            calls[1]()
            hs[0].synchronize()
            hs[1].synchronize()
        st.synchronize()
        got[mode] = out.cpu().numpy().copy()
        for h in hs:
            h.close()
    assert np.array_equal(got["0"], got["force"]), "paired and single passes differ"
    print("pair_launch: %d pass pairs each way, bitsets equal, %d bits set" % (n, int(np.unpackbits(got["0"].view(np.uint8)).sum())))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        stats(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--timeline":
        timeline(sys.argv[2])
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 300)

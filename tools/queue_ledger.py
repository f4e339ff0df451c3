#!/usr/bin/env python
"""Queue ledger of the pipelined step: where the IN-ORDER QUEUE TIME of one batch's launch chain goes, from a
`rocprofv3 --kernel-trace` of `python bench.py --gpus 1 --steps S --warmup W` (tools/step_account.py reads the same trace for SIMD time).

With few hardware queues every queue runs whole per-batch chains one after another, so the step time is bounded below by
(queue time of one chain) / (number of queues).  This table tests that reading:

  * per kernel family: launches per batch, mean duration, queue time per batch and its share of  queues x step time;
  * the sum of one chain's durations against  queues x step time  (equal = the queues never wait; smaller = they idle);
  * per queue, the share of the window in which one of its chains is open (first start to last end of a chain);
  * the gap between dependent nodes of one slot, as the trace has it.  Inside a captured graph the profiler stamps a node's start at
    its predecessor's end, so the launch gap of a dependent node is INSIDE its duration and the stamped gap is ~0: the column
    says whether that is the case in this trace; gaps that do show are queue hand-overs;
  * the LM kernel next to stage A's refit kernel (and the fused kernel, once it replaces both).

A chain = the dispatches of one stream from one `--tail` kernel (the step's last node) to the next.

usage: queue_ledger.py <kernel_trace.csv> --steps S [--trim 0.15] [--out table.txt]"""
import argparse
import collections
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_account import MARKERS, base_name, family  # noqa: E402

WATCH = ("ransac_joint_lm_kernel", "ransac_joint_lm_kind_kernel", "ransac_single_finish_kernel", "pose_lm_finish_a_kernel",
         "pose_lm_finish_a_kind_kernel", "ransac_single_score_sreg_kernel", "ransac_joint_finish_kernel")


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        if r.get("Kind") not in (None, "KERNEL_DISPATCH"):
            continue
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Stream_Id"], r["Kernel_Name"]))
    rows.sort()
    return rows


def ledger(rows, steps, trim, tail):
    marks = [r[0] for r in rows if any(m in r[4] for m in MARKERS)]
    if len(marks) < 8:
        raise SystemExit("no once-per-step marker kernel (%s) in the trace" % " / ".join(MARKERS))
    if steps:
        marks = marks[-int(steps):]
    a, b = int(trim * len(marks)), len(marks) - 1 - int(trim * len(marks))
    lo, hi, nsteps = marks[a], marks[b], b - a
    step_ns = (hi - lo) / float(nsteps)
    streams = collections.defaultdict(list)
    for r in rows:
        streams[(r[2], r[3])].append(r)
    chains = []                                                 # (queue, [dispatch, ...]) wholly inside the window
    for (q, _), rs in streams.items():
        cur = []
        for r in rs:
            cur.append(r)
            if tail in r[4]:
                if len(cur) > 1 and cur[0][0] >= lo and cur[-1][1] <= hi:
                    chains.append((q, cur))
                cur = []
    if not chains:
        raise SystemExit("no complete chain ending in %r inside the window" % tail)
    length = collections.Counter(len(c) for _, c in chains).most_common(1)[0][0]
    chains = [(q, c) for q, c in chains if len(c) == length]     # the step's chain (drops set-up launches that precede the first tail)
    queues = sorted({q for q, _ in chains})
    fam_dur, fam_n = collections.defaultdict(float), collections.defaultdict(int)
    ker_dur = collections.defaultdict(list)
    gaps, chain_sum, chain_span = [], [], []
    open_ns = collections.defaultdict(float)
    for q, c in chains:
        chain_sum.append(sum(e - s for s, e, *_ in c))
        chain_span.append(c[-1][1] - c[0][0])
        open_ns[q] += c[-1][1] - c[0][0]
        for i, (s, e, _, _, name) in enumerate(c):
            fam_dur[family(name)] += e - s
            fam_n[family(name)] += 1
            if base_name(name) in WATCH:
                ker_dur[base_name(name)].append(e - s)
            if i:
                gaps.append(s - c[i - 1][1])
    return dict(lo=lo, hi=hi, nsteps=nsteps, step_ns=step_ns, chains=chains, length=length, queues=queues, fam_dur=fam_dur, fam_n=fam_n,
                ker_dur=ker_dur, gaps=gaps, chain_sum=chain_sum, chain_span=chain_span, open_ns=open_ns)


def report(L, out):
    w = out.write
    n, nq = len(L["chains"]), len(L["queues"])
    budget = nq * L["step_ns"]
    mean = lambda v: sum(v) / max(1, len(v))
    w("window %.1f ms = %d steps -> %.4f ms per step; %d whole chains of %d launches on %d hardware queues\n"
      % ((L["hi"] - L["lo"]) * 1e-6, L["nsteps"], L["step_ns"] * 1e-6, n, L["length"], nq))
    w("queue budget of one batch = queues x step time = %.4f ms\n\n" % (budget * 1e-6))
    w("%-40s %9s %12s %14s %8s\n" % ("family", "per_batch", "mean_us", "queue_ms/batch", "share"))
    for fam in sorted(L["fam_dur"], key=lambda f: -L["fam_dur"][f]):
        d, k = L["fam_dur"][fam], L["fam_n"][fam]
        w("%-40s %9.1f %12.1f %14.4f %7.1f%%\n" % (fam, k / float(n), d / k * 1e-3, d / n * 1e-6, 100.0 * d / n / budget))
    cs = mean(L["chain_sum"])
    w("%-40s %9d %12s %14.4f %7.1f%%   (sum of one chain's durations / queue budget)\n" % ("sum", L["length"], "", cs * 1e-6, 100.0 * cs / budget))
    w("chain span (first start to last end)     mean %.4f ms, min %.4f, max %.4f\n"
      % (mean(L["chain_span"]) * 1e-6, min(L["chain_span"]) * 1e-6, max(L["chain_span"]) * 1e-6))
    w("queue has a chain open                   " + ", ".join("queue %s: %.1f%%" % (q, 100.0 * L["open_ns"][q] / (L["hi"] - L["lo"])) for q in L["queues"])
      + "   (of the window; whole chains only, so the two cut at the window's ends are missing)\n")
    g = sorted(L["gaps"])
    w("gap between dependent nodes of a slot    mean %.2f us, median %.2f us, p99 %.2f us, max %.2f us, zero in %.1f%% of %d\n"
      % (mean(g) * 1e-3, g[len(g) // 2] * 1e-3, g[int(0.99 * (len(g) - 1))] * 1e-3, g[-1] * 1e-3, 100.0 * sum(1 for x in g if x <= 0) / len(g), len(g)))
    w("  (a zero gap is the profiler stamping a graph node's start at its predecessor's end: the launch gap is inside the duration)\n\n")
    w("%-40s %9s %12s %12s %12s\n" % ("kernel", "launches", "mean_us", "min_us", "max_us"))
    for k in WATCH:
        v = L["ker_dur"].get(k)
        if v:
            w("%-40s %9d %12.1f %12.1f %12.1f\n" % (k, len(v), mean(v) * 1e-3, min(v) * 1e-3, max(v) * 1e-3))
        else:
            w("%-40s %9d   (no such node in the step)\n" % (k, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--steps", type=float, default=0, help="steps of the timed region (the last launches of the once-per-step marker kernel)")
    ap.add_argument("--trim", type=float, default=0.15)
    ap.add_argument("--tail", default="poison_records", help="substring of the step's last kernel: a chain ends with it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = load(a.trace)
    out = open(a.out, "w") if a.out else sys.stdout
    out.write("# tools/queue_ledger.py %s --steps %g --trim %g   (%d dispatches)\n" % (a.trace.split("/")[-1], a.steps, a.trim, len(rows)))
    report(ledger(rows, a.steps, a.trim, a.tail), out)


if __name__ == "__main__":
    main()

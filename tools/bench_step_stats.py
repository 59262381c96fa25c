"""Times the step-statistics launch (csrc/step_stats.hip, stego_amd.step_stats.StepStats) against the chain it replaces, at the shipped
configuration's shapes: feature_samples S = 11, neg_samples 5, batch B = 16 and 32, i.e. two cd tensors of B * S^4 floats and one of
5 * B * S^4, the last a view behind the first two as cd[2:].flatten(0, 1) is; nine loss scalars ride along.

Per batch size, on the same visit, variants alternating inside every round, medians over the rounds:
  stats        StepStats.record(with_hist=False)         against   means3      three .mean() launches (what every step pays today)
  stats_hist   StepStats.record(with_hist=True)          against   numpy_hist  three .cpu() copies + np.histogram on TensorBoard's bins
                                                                               (what the reference pays on a histogram step; host time)
Device time and host enqueue time are measured apart, as tools/bench_optim.py does: a window of back-to-back calls between two events
(device us per call) with the host clock around the same window and no synchronise (enqueue us per call), and the two stats variants
once more as a captured graph replayed (device us per call without the host in between).
`--trainer-rounds N` runs tools/exp/trainer_step_time.py native_probes=True with and without train_log=True, N fresh processes each,
alternating: the cached-token training_step at B = 32 (the flag off is the parent commit's step: nothing else differs).

    python tools/bench_step_stats.py --out profiles/step_stats_bench.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stego_amd.step_stats import StepStats, default_bins  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12          # bytes/s: the device copy rate the README measures rooflines against
S, NEG, N_SCALARS = 11, 5, 9


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_cd(B):
    """cd-like values (tanh of a normal: inside (-1, 1), most mass in +-[0.01, 1]) in one buffer [2 + NEG, B, S^4]-shaped as the loss
    returns them: the negatives are the view behind the first two blocks."""
    g = torch.Generator(device=DEV).manual_seed(B)
    n = B * S ** 4
    buf = torch.tanh(0.4 * torch.randn((2 + NEG) * n, device=DEV, generator=g))     # (B * S^4 * 4 bytes is a multiple of 16 at these B)
    return [buf[:n], buf[n:2 * n], buf[2 * n:]]


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    host = (time.perf_counter() - t0) * 1e6 / n
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n, host


def bench_batch(B, args):
    cd = make_cd(B)
    scalars = list(torch.randn(N_SCALARS, device=DEV).unbind(0))
    bins = default_bins()
    stats = {False: StepStats(N_SCALARS, 16, DEV), True: StepStats(N_SCALARS, 16, DEV)}
    sink = {}

    def means3():
        sink["m"] = (cd[0].mean(), cd[1].mean(), cd[2].mean())

    def numpy_hist():
        sink["h"] = [np.histogram(t.cpu().numpy(), bins=bins)[0] for t in cd]

    calls = {"stats": lambda: stats[False].record(cd, scalars, False), "stats_hist": lambda: stats[True].record(cd, scalars, True),
             "means3": means3}
    for fn in list(calls.values()) + [numpy_hist]:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two sides agree before anything is timed
    rec = stats[True].drain()[-1]
    for t, m, h in zip(rec["tensors"], sink["m"], sink["h"]):
        assert abs(t["mean"] - float(m)) <= 1e-5 * max(abs(float(m)), 1e-3), (t["mean"], float(m))
        assert (t["counts"].astype(np.int64) == h).all()
    occupied = [int((t["counts"] > 0).sum()) for t in rec["tensors"]]
    res = {k: {"device_us": [], "host_us": []} for k in calls}
    res["numpy_hist"] = {"host_us": []}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            d, h = window(fn, args.window)
            res[k]["device_us"].append(d)
            res[k]["host_us"].append(h)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.hist_calls):
            numpy_hist()
        res["numpy_hist"]["host_us"].append((time.perf_counter() - t0) * 1e6 / args.hist_calls)
    out = {"B": B, "elements": [int(t.numel()) for t in cd], "occupied_buckets": occupied, "window": args.window, "rounds": args.rounds}
    for k, r in res.items():
        out[k] = {m: round(med(x), 2) for m, x in r.items()}
        out[k].update({m + "_min": round(min(x), 2) for m, x in r.items()})
    for with_hist, name in ((False, "stats"), (True, "stats_hist")):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.window):
                stats[with_hist].record(cd, scalars, with_hist)
        times = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            graph.replay()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.window)
        nbytes = 4 * sum(int(t.numel()) for t in cd)
        plan = stats[with_hist].launch_plan([t.numel() for t in cd], with_hist)
        out[name].update({"graph_replay_us": round(med(times), 2), "graph_replay_us_min": round(min(times), 2), "bytes": nbytes,
                          "us_at_copy_rate": round(nbytes / COPY_RATE * 1e6, 2),
                          "frac_of_copy_rate_graph_replay": round(nbytes / COPY_RATE / (med(times) * 1e-6), 4),
                          "grid": plan["grid"], "chunk": plan["chunk"], "record_bytes": plan["record_bytes"]})
    out["stats_vs_means3_device"] = round(out["means3"]["device_us"] / out["stats"]["device_us"], 2)
    out["stats_vs_means3_host"] = round(out["means3"]["host_us"] / out["stats"]["host_us"], 2)
    out["stats_hist_vs_numpy_hist_host_over_device"] = round(out["numpy_hist"]["host_us"] / out["stats_hist"]["device_us"], 1)
    return out


def trainer_steps(rounds):
    script = os.path.join(ROOT, "tools", "exp", "trainer_step_time.py")
    out = {"train_log=False": [], "train_log=True": []}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(rounds):
            for flag in (False, True):
                cmd = [sys.executable, script, "native_probes=True"] + (["train_log=True", "output_root=%s" % tmp] if flag else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
                m = re.search(r"enqueue ([0-9.]+) ms, wall ([0-9.]+) ms", r.stdout)
                if r.returncode != 0 or not m:
                    raise RuntimeError("trainer_step_time.py failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                out["train_log=%s" % flag].append({"enqueue_ms": float(m.group(1)), "wall_ms": float(m.group(2))})
                print("trainer step, train_log=%s: %s" % (flag, out["train_log=%s" % flag][-1]), flush=True)
    res = {"what": "tools/exp/trainer_step_time.py native_probes=True (cached tokens, B = 32 pairs, 64 steps), one fresh process per run",
           "runs": out,
           "wall_ms": {k: med([x["wall_ms"] for x in v]) for k, v in out.items()},
           "enqueue_ms": {k: med([x["enqueue_ms"] for x in v]) for k, v in out.items()}}
    off, on = [x["wall_ms"] for x in out["train_log=False"]], [x["wall_ms"] for x in out["train_log=True"]]
    res["spread_ms"] = {"train_log=False": round(max(off) - min(off), 4), "train_log=True": round(max(on) - min(on), 4)}
    res["on_minus_off_wall_ms"] = round(res["wall_ms"]["train_log=True"] - res["wall_ms"]["train_log=False"], 4)
    res["on_not_slower_beyond_spread"] = bool(res["on_minus_off_wall_ms"] <= max(res["spread_ms"].values()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hist-calls", type=int, default=2, help="numpy histogram chains per round")
    ap.add_argument("--trainer-rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_stats_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_step_stats needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "variants alternate inside every round, medians over the rounds; device us: a window of back-to-back calls between "
                     "two events; host us: the clock around the same window, no synchronise; numpy_hist: wall clock, it waits for its copies"}
    for B in (16, 32):
        rec["B%d" % B] = bench_batch(B, args)
        print(json.dumps({"B%d" % B: rec["B%d" % B]}), flush=True)
    if args.trainer_rounds > 0:
        rec["training_step"] = trainer_steps(args.trainer_rounds)
    rec["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Times the fused Adam step (csrc/optim_step.hip, stego_amd.optim.FusedAdam) against the chain it replaces, on the two trainable sets
of the trainer: the ViT-S nonlinear head plus both probes (205 547 floats in 9 tensors) and the ViT-B one (702 059).

Per set, four variants of one parameter update, each on its own copy of the parameters, all fed the same gradients:
  torch_bucket    today's data-parallel path: FlatGradReducer.zero_grad() (one launch over the bucket) + three torch.optim.Adam.step()
  torch_zero_grad today's single-process path: three optimizer.zero_grad() (set_to_none: host work only; the gradient tensors are
                  re-attached inside the timed region, nine host assignments that stand in for the backward) + three step()
  fused           FusedAdam.step() with the zeroing in the kernel
  fused_no_zero   FusedAdam.step() with zero_grads off + the bucket's zero_() launch (cfg.native_optim_zero = False)
(inside a timed window the zeroing variants step on zero gradients after the first call; Adam's launches do not depend on the data)
and three ways of timing them, variants alternating inside every round, medians over the rounds:
  resident  a window of `--window` back-to-back calls between two events: device us per call with the arrays cache-resident (the
            window's total is 0.8 .. 23 MB), and the host clock around the same window without a synchronise: enqueue us per call
  graph     (fused only) `--window` steps captured in one graph and replayed: device us per step without the host in between
  evicted   single calls, a 512 MB buffer rewritten before each (the state was last touched a whole training step ago): device us by
            events around the one call, host us by a clock around it
`--trainer-rounds N` also runs tools/exp/trainer_step_time.py native_probes=True with and without native_optim=True, N times each,
alternating, every run a fresh process.

    python tools/bench_optim.py --out profiles/optim_bench.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stego_amd import ddp  # noqa: E402
from stego_amd.optim import FusedAdam  # noqa: E402

DEV = torch.device("cuda:0")
COPY_RATE = 6.29e12          # bytes/s: the device copy rate the README measures rooflines against
LRS = (5e-4, 5e-3, 5e-3)


def shapes(C, K=70, n=27):
    """The trainable tensors of LitUnsupervisedSegmenter in the order of its three optimizers: cluster1, cluster2 (nonlinear), the
    linear probe, the cluster probe."""
    return [[(K, C, 1, 1), (K,), (C, C, 1, 1), (C,), (K, C, 1, 1), (K,)], [(n, K, 1, 1), (n,)], [(n, K)]]


def make_params(C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [[torch.nn.Parameter(torch.randn(s, device=DEV, generator=g) * 0.05) for s in grp] for grp in shapes(C)]


class Variant:
    def __init__(self, name, C, grads):
        self.name = name
        self.params = make_params(C, 0)
        flat = [p for grp in self.params for p in grp]
        self.grad_src = grads
        if name.startswith("fused"):
            self.opt = FusedAdam([{"params": grp, "lr": lr} for grp, lr in zip(self.params, LRS)], zero_grads=name == "fused")
            self.bucket = self.opt.bucket
        else:
            self.adams = [torch.optim.Adam(grp, lr=lr) for grp, lr in zip(self.params, LRS)]
            if name == "torch_bucket":
                self.bucket = ddp.FlatGradReducer(flat)
            else:
                self.bucket = None
                self.held, off = [], 0
                for p in flat:
                    self.held.append(torch.empty_like(p))
                    off += p.numel()
        self.flat = flat

    def feed(self):
        """Untimed: what the backward leaves behind."""
        if self.bucket is not None:
            self.bucket.flat.copy_(self.grad_src)
        else:
            off = 0
            for h in self.held:
                h.copy_(self.grad_src[off:off + h.numel()].view_as(h))
                off += h.numel()

    def call(self):
        """The update, then the zeroing that opens the next step (the trainer zeroes first: the same launches, and in this order
        every variant steps on what feed() left)."""
        if self.name == "fused":
            self.opt.step()
        elif self.name == "fused_no_zero":
            self.opt.step()
            self.opt.zero_grad()
        elif self.name == "torch_bucket":
            for a in self.adams:
                a.step()
            self.bucket.zero_grad()
        else:
            for p, h in zip(self.flat, self.held):
                p.grad = h
            for a in self.adams:
                a.step()
            for a in self.adams:
                a.zero_grad()


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def bench_set(C, args):
    numel = sum(int(torch.Size(s).numel()) for grp in shapes(C) for s in grp)
    grads = torch.randn(numel, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 1e-3
    variants = [Variant(n, C, grads) for n in ("torch_bucket", "torch_zero_grad", "fused", "fused_no_zero")]
    evict = torch.zeros(512 * 2 ** 20 // 4, device=DEV)
    # warm-up (code objects, torch's foreach paths, the allocator) that is also the comparison of results: every variant starts from
    # the same parameters and takes the same `--warmup` steps on the same gradients, so the parameters agree to Adam's rounding
    for v in variants:
        for k in range(args.warmup):
            v.grad_src = grads * (1.0 + 0.1 * k)
            v.feed()
            v.call()
        v.grad_src = grads
    torch.cuda.synchronize()
    ref = torch.cat([p.detach().reshape(-1) for p in variants[0].flat])
    agree = {v.name: float((torch.cat([p.detach().reshape(-1) for p in v.flat]) - ref).abs().max()) for v in variants[1:]}
    res = {v.name: {"resident_us": [], "resident_host_us": [], "evicted_us": [], "evicted_host_us": []} for v in variants}
    for _ in range(args.rounds):
        for v in variants:                                # resident: one window
            v.feed()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.window):
                v.call()
            b.record()
            host = (time.perf_counter() - t0) * 1e6 / args.window
            b.synchronize()
            res[v.name]["resident_us"].append(a.elapsed_time(b) * 1e3 / args.window)
            res[v.name]["resident_host_us"].append(host)
        for _ in range(args.evicted_calls):               # evicted: single calls
            for v in variants:
                v.feed()
                evict.add_(1.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                a.record()
                v.call()
                b.record()
                host = (time.perf_counter() - t0) * 1e6
                b.synchronize()
                res[v.name]["evicted_us"].append(a.elapsed_time(b) * 1e3)
                res[v.name]["evicted_host_us"].append(host)
    torch.cuda.synchronize()
    out = {"elements": numel, "tensors": len(variants[0].flat), "window": args.window, "rounds": args.rounds,
           "evicted_calls": args.rounds * args.evicted_calls}
    for name, r in res.items():
        out[name] = {k: round(med(x), 2) for k, x in r.items()}
        out[name].update({k + "_min": round(min(x), 2) for k, x in r.items()})
    grid, chunk, n_chunks = variants[2].opt.plan()
    nbytes = 32 * numel                                   # g, m, v, p read; m, v, p and the zeroed g written
    out["fused"].update({"grid": grid, "chunk": chunk, "bytes": nbytes, "us_at_copy_rate": round(nbytes / COPY_RATE * 1e6, 2),
                         "frac_of_copy_rate_resident": round(nbytes / COPY_RATE / (out["fused"]["resident_us"] * 1e-6), 4),
                         "frac_of_copy_rate_evicted": round(nbytes / COPY_RATE / (out["fused"]["evicted_us"] * 1e-6), 4)})
    for name, d in agree.items():
        out[name]["max_abs_param_diff_vs_torch_bucket_after_warmup"] = d
    out["warmup_steps_compared"] = args.warmup
    out["steps_taken"] = int(variants[2].opt.steps[0])
    # the launch alone: `--window` fused steps captured in one graph (a straight line of kernels), replayed - no host work between
    # the launches, so this is the device time per step with the arrays cache-resident where the eager window is bound by the enqueue
    fused = variants[2]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.window):
            fused.opt.step()
    times = []
    for _ in range(args.rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / args.window)
    out["fused"]["graph_replay_us"] = round(med(times), 2)
    out["fused"]["graph_replay_us_min"] = round(min(times), 2)
    out["fused"]["frac_of_copy_rate_graph_replay"] = round(nbytes / COPY_RATE / (out["fused"]["graph_replay_us"] * 1e-6), 4)
    for k in ("resident_us", "resident_host_us", "evicted_us", "evicted_host_us"):
        out["fused_below_both_torch_chains_" + k] = bool(out["fused"][k] < min(out["torch_bucket"][k], out["torch_zero_grad"][k]))
    return out


def trainer_steps(rounds):
    script = os.path.join(ROOT, "tools", "exp", "trainer_step_time.py")
    out = {"native_optim=False": [], "native_optim=True": []}
    for _ in range(rounds):
        for flag in (False, True):
            cmd = [sys.executable, script, "native_probes=True"] + (["native_optim=True"] if flag else [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
            m = re.search(r"enqueue ([0-9.]+) ms, wall ([0-9.]+) ms", r.stdout)
            if r.returncode != 0 or not m:
                raise RuntimeError("trainer_step_time.py failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            out["native_optim=%s" % flag].append({"enqueue_ms": float(m.group(1)), "wall_ms": float(m.group(2))})
            print("trainer step, native_optim=%s: %s" % (flag, out["native_optim=%s" % flag][-1]), flush=True)
    return {"what": "tools/exp/trainer_step_time.py native_probes=True (cached tokens, B = 32 pairs, 64 steps), one fresh process per run",
            "runs": out,
            "wall_ms": {k: med([x["wall_ms"] for x in v]) for k, v in out.items()},
            "enqueue_ms": {k: med([x["enqueue_ms"] for x in v]) for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--evicted-calls", type=int, default=15, help="single evicted calls per variant and round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trainer-rounds", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim needs the MI355X"
    t0 = time.time()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "variants alternate inside every round, medians over the rounds; resident: windows of back-to-back calls, arrays "
                     "cache-resident; evicted: single calls behind a 512 MB rewrite"}
    for name, C in (("vit_small_head_and_probes", 384), ("vit_base_head_and_probes", 768)):
        rec[name] = bench_set(C, args)
        print(json.dumps({name: rec[name]}), flush=True)
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

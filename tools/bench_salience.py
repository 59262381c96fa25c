"""The salience-guided coordinate draws (cfg.use_salience): the one-launch native draw (stego_salience_coords, with the torch.rand
calls that feed it) against the chain it replaces, modules.sample_nonzero_locations x 2, at B = 16 and 32, 224 x 224 masks, S = 11.

    python tools/bench_salience.py [--iters 50]      -> profiles/salience_bench.json, and the same JSON on one line

Device time: CUDA events around back-to-back calls; host time: wall clock per call with a synchronisation only at the end (the torch
chain synchronises by itself, 2 * B times per call: torch.nonzero and the boolean indexing of every image)."""
import argparse
import json
import os
import sys
import time
from os.path import join

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stego_amd import capi  # noqa: E402
from stego_amd.modules import sample_nonzero_locations  # noqa: E402


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e6 / iters
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 2), round(host, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, S = 224, 11
    rows = []
    for B in (16, 32):
        g = torch.Generator(device=dev).manual_seed(B)
        m1 = (torch.rand(B, H, H, device=dev, generator=g) < 0.3).float()
        m2 = (torch.rand(B, H, H, device=dev, generator=g) < 0.3).float()
        shape = [B, S, S, 2]

        def native():
            reg1 = torch.rand(shape, device=dev) * 2 - 1
            reg2 = torch.rand(shape, device=dev) * 2 - 1
            u = torch.rand([2, B, S, S, 3], device=dev)
            u_mix = torch.rand([B, S, S], device=dev)
            return capi.salience_coords(m1, m2, u, u_mix, reg1, reg2)

        def kernel_only(u=torch.rand([2, B, S, S, 3], device=dev), u_mix=torch.rand([B, S, S], device=dev),
                        reg=torch.rand(shape, device=dev)):
            return capi.salience_coords(m1, m2, u, u_mix, reg, reg)

        def chain():
            return sample_nonzero_locations(m1, shape), sample_nonzero_locations(m2, shape)

        n_dev, n_host = timed(native, a.iters)
        k_dev, k_host = timed(kernel_only, a.iters)
        c_dev, c_host = timed(chain, a.iters)
        rows.append(dict(B=B, H=H, W=H, S=S, native_device_us=n_dev, native_host_us=n_host, native_kernel_call_device_us=k_dev,
                         native_kernel_call_host_us=k_host, torch_chain_device_us=c_dev, torch_chain_host_us=c_host,
                         speedup_device=round(c_dev / n_dev, 2), speedup_host=round(c_host / n_host, 2)))
    result = dict(tool="bench_salience", rows=rows)
    out = join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "salience_bench.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()

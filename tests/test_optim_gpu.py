"""The fused Adam step on the GPU (include/stego_optim.h, stego_amd.optim.FusedAdam) against a float64 restatement of Adam that runs on
the CPU: three groups with their own learning rates over segments of 1 .. chunk + 1 elements at every alignment, three gradient
regimes of 25 steps, the fused zeroing, determinism, graph capture, and the trainer with cfg.native_optim.

Bounds after T steps (one rounding of p per step plus a few roundings inside the update; torch.optim.Adam in fp32 stays inside them):
    parameters  T * (2^-24 * max|p| + 2^-20 * lr)        exp_avg  T * 2^-23 * max|g|        exp_avg_sq  T * 2^-23 * max g^2
"""
import warnings

import numpy as np
import pytest
import torch

from stego_amd import capi
from stego_amd.optim import FusedAdam

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="DinoFeaturizer")

DEV = "cuda"
T = 25
LRS = (5e-4, 5e-3, 5e-3)
BETAS, EPS = (0.9, 0.999), 1e-8
CHUNK = capi.ADAM_CHUNK
# (elements, float offset of the parameter in one base allocation, group, trainable).  Gradient offsets follow the order of the trainable
# segments, packed: 0, 1025, 1095, 1098, 3015, 3016, 3020 - three odd, one more that is no multiple of 4.  All four addresses 16-byte
# aligned (the float4 path): the chunk + 1 segment (a whole chunk, then a chunk of one element) and the 5 (one float4, one tail element);
# the 4 has a 16-byte aligned gradient and a parameter that is not; the 1917 has an odd parameter address.
SEGMENTS = [(CHUNK + 1, 0, 0, True), (70, 1028, 0, True), (7, 1098, 0, False), (3, 1108, 0, True),
            (1917, 1113, 1, True), (1, 3032, 1, True), (4, 3034, 2, True), (5, 3040, 2, True)]
BASE_LEN = 3048
assert CHUNK == 1024 and sorted(n for n, _, _, tr in SEGMENTS if tr) == [1, 3, 4, 5, 70, CHUNK + 1, 1917]


def _build(seed=0, zero_grads=True, scale=1.0):
    """(fused, base, params): the parameters are views into `base`, the floats between them guards that no step may touch."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(BASE_LEN, generator=g) * scale).to(DEV)
    params = []
    for n, off, _, trainable in SEGMENTS:
        params.append(torch.nn.Parameter(base[off:off + n], requires_grad=trainable))
    groups = [{"params": [p for p, s in zip(params, SEGMENTS) if s[2] == gi], "lr": LRS[gi], "betas": BETAS, "eps": EPS} for gi in range(3)]
    return FusedAdam(groups, zero_grads=zero_grads), base, params


def _trainable(params):
    return [(p, s) for p, s in zip(params, SEGMENTS) if s[3]]


def _gradients(regime, seed=1):
    """float32 [T, numel] in the bucket's order."""
    numel = sum(n for n, _, _, tr in SEGMENTS if tr)
    g = torch.randn(T, numel, generator=torch.Generator().manual_seed(seed))
    if regime == "1e-3":
        return g * 1e-3
    if regime == "1":
        return g
    g = g * 1e-6
    g[:, ::3] = 0.0                                   # every third element exactly 0 in every step: v = 0 there, eps alone divides
    return g


def adam64(p, grads, lr, steps_before=0, m=None, v=None):
    """Adam in float64: p [n], grads [T, n] -> (p, m, v) after the T steps."""
    p = p.astype(np.float64).copy()
    m = np.zeros_like(p) if m is None else m.astype(np.float64).copy()
    v = np.zeros_like(p) if v is None else v.astype(np.float64).copy()
    b1, b2 = BETAS
    for i, g in enumerate(grads.astype(np.float64)):
        t = steps_before + i + 1
        m += (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        p -= (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + EPS)
    return p, m, v


def _state(fused, p):
    a = fused._state_off[id(p)]
    return fused.exp_avg[a:a + p.numel()].cpu().numpy(), fused.exp_avg_sq[a:a + p.numel()].cpu().numpy()


_CASES = {}


def _case(regime):
    """One 25-step run per regime, shared by the tests that read it: the fused result, the oracle and torch's own fp32 result."""
    if regime in _CASES:
        return _CASES[regime]
    fused, base, params = _build()
    base0 = base.cpu().clone()
    grads = _gradients(regime)
    dev_grads = grads.to(DEV)
    for t in range(T):
        fused.bucket.flat.copy_(dev_grads[t])
        fused.step()
    torch.cuda.synchronize()
    out = {"fused": fused, "base0": base0, "base": base.cpu(), "params": params, "grads": grads, "segs": []}
    off = 0
    for p, (n, boff, gi, _) in _trainable(params):
        g = grads[:, off:off + n].numpy()
        p0 = base0[boff:boff + n].numpy()
        want = adam64(p0, g, LRS[gi])
        tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))                 # torch.optim.Adam in fp32 on the CPU, same input
        topt = torch.optim.Adam([tp], lr=LRS[gi], betas=BETAS, eps=EPS)
        for t in range(T):
            tp.grad = torch.from_numpy(g[t].copy())
            topt.step()
        m, v = _state(fused, p)
        out["segs"].append(dict(n=n, gi=gi, g=g, p0=p0, want=want, got=(p.detach().cpu().numpy(), m, v),
                                torch=(tp.detach().numpy(), topt.state[tp]["exp_avg"].numpy(), topt.state[tp]["exp_avg_sq"].numpy())))
        off += n
    _CASES[regime] = out
    return out


@pytest.mark.parametrize("regime", ["1e-3", "1", "1e-6"])
def test_25_steps_against_float64(regime):
    c = _case(regime)
    assert c["fused"].steps.tolist() == [T, T, T]
    lines = []
    for s in c["segs"]:
        lr, g = LRS[s["gi"]], s["g"]
        pmax = max(np.abs(s["want"][0]).max(), np.abs(s["p0"]).max())
        bounds = (T * (2.0 ** -24 * pmax + 2.0 ** -20 * lr), T * 2.0 ** -23 * np.abs(g).max(), T * 2.0 ** -23 * (g.astype(np.float64) ** 2).max())
        for name, got, want, ref, bound in zip(("param", "exp_avg", "exp_avg_sq"), s["got"], s["want"], s["torch"], bounds):
            assert np.isfinite(got).all(), (regime, s["n"], name)
            err, terr = np.abs(got - want).max(), np.abs(ref - want).max()
            lines.append("n=%d %s: err %.3g bound %.3g, torch fp32 err %.3g (ours / torch %.2f)"
                         % (s["n"], name, err, bound, terr, err / terr if terr > 0 else float("inf") if err > 0 else 1.0))
            print(regime, lines[-1])
            assert err <= bound, (regime, lines[-1])
        if regime == "1e-6":                          # g = 0 in every step: the element stays put and its state stays 0
            off = sum(x["n"] for x in c["segs"][:c["segs"].index(s)])
            still = (np.arange(off, off + s["n"]) % 3) == 0
            assert np.array_equal(s["got"][0][still], s["p0"][still]) and not s["got"][1][still].any() and not s["got"][2][still].any()
        assert np.abs(s["got"][0] - s["p0"]).max() > 0.5 * lr or regime == "1e-6"         # the parameters did move


@pytest.mark.parametrize("regime", ["1e-3", "1e-6"])
def test_nothing_outside_the_segments_changes(regime):
    c = _case(regime)
    touched = torch.zeros(BASE_LEN, dtype=torch.bool)
    for n, off, _, trainable in SEGMENTS:
        if trainable:
            touched[off:off + n] = True
    assert torch.equal(c["base"][~touched], c["base0"][~touched])             # the guards between the segments and the frozen parameter
    fused = c["fused"]
    pad = torch.ones(fused.exp_avg.numel(), dtype=torch.bool)
    for p, _ in _trainable(c["params"]):
        a = fused._state_off[id(p)]
        pad[a:a + p.numel()] = False
    assert not fused.exp_avg.cpu()[pad].any() and not fused.exp_avg_sq.cpu()[pad].any()
    assert int(fused._ticket) == 0                                             # the last workgroup put the ticket back
    assert fused._counters.cpu()[3:8].tolist() == [0] * 5


def test_fused_zeroing():
    grads = _gradients("1e-3", seed=3).to(DEV)
    fused, base, params = _build()
    base0 = base.cpu().clone()
    views = [p.grad.data_ptr() for p, _ in _trainable(params)]
    for t in range(2):
        fused.bucket.flat.copy_(grads[t])
        fused.step()
        assert not fused.bucket.flat.any()                                     # ready for the next backward
    assert [p.grad.data_ptr() for p, _ in _trainable(params)] == views
    lo, hi = fused.bucket.flat.data_ptr(), fused.bucket.flat.data_ptr() + 4 * fused.bucket.flat.numel()
    assert all(lo <= v < hi for v in views)
    off = 0
    for p, (n, boff, gi, _) in _trainable(params):                            # the second step saw the fresh gradients, not zeros
        want = adam64(base0[boff:boff + n].numpy(), grads[:2, off:off + n].cpu().numpy(), LRS[gi])[0]
        bound = 2 * (2.0 ** -24 * np.abs(want).max() + 2.0 ** -20 * LRS[gi])
        assert np.abs(p.detach().cpu().numpy() - want).max() <= bound, n
        off += n
    keep, kbase, kparams = _build(zero_grads=False)
    keep.bucket.flat.copy_(grads[0])
    keep.step()
    assert torch.equal(keep.bucket.flat, grads[0])                             # zero_grads off: the bucket is left bit for bit
    fused2, base2, _ = _build()
    fused2.bucket.flat.copy_(grads[0])
    fused2.step()
    assert torch.equal(kbase, base2)                                           # and the update is the same either way


def test_one_group_alone():
    grads = _gradients("1e-3", seed=4).to(DEV)
    fused, base, params = _build()
    base0 = base.clone()
    fused.bucket.flat.copy_(grads[0])
    fused.groups[1].step()
    assert fused.steps.tolist() == [0, 1, 0]
    off = 0
    for p, (n, boff, gi, _) in _trainable(params):
        changed = not torch.equal(base[boff:boff + n], base0[boff:boff + n])
        assert changed == (gi == 1), n
        assert torch.equal(fused.bucket.flat[off:off + n], grads[0][off:off + n]) == (gi != 1)      # only its own gradients are zeroed
        off += n
    fused.groups[0].zero_grad()
    fused.groups[2].zero_grad()
    assert not fused.bucket.flat.any()


def test_two_optimizers_end_bitwise_equal():
    grads = _gradients("1", seed=5).to(DEV)
    ends = []
    for _ in range(2):
        fused, base, _ = _build()
        for t in range(5):
            fused.bucket.flat.copy_(grads[t])
            fused.step()
        ends.append((base.cpu(), fused.exp_avg.cpu(), fused.exp_avg_sq.cpu(), fused.steps.cpu()))
    for a, b in zip(*ends):
        assert torch.equal(a, b)


def test_three_steps_in_one_graph():
    """copy, step, copy, step, copy, step as one captured line of kernels: replays match the same steps run eagerly bit for bit, the
    counters advance by 3 per replay (they live on the device: nothing of the step is frozen into the graph)."""
    grads = _gradients("1e-3", seed=6).to(DEV)
    eager, ebase, _ = _build()
    graphed, gbase, _ = _build()
    for f in (eager, graphed):                                                 # one step outside the capture: the code object is loaded
        f.bucket.flat.copy_(grads[0])
        f.step()
    feed = torch.zeros(3, grads.shape[1], device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(3):
            graphed.bucket.flat.copy_(feed[k])
            graphed.step()
    assert graphed.steps.tolist() == [1, 1, 1]                                 # capturing ran nothing
    for r in range(2):
        feed.copy_(grads[1 + 3 * r:4 + 3 * r])
        graph.replay()
        for k in range(3):
            eager.bucket.flat.copy_(grads[1 + 3 * r + k])
            eager.step()
        assert graphed.steps.tolist() == [4 + 3 * r] * 3
    torch.cuda.synchronize()
    assert torch.equal(gbase, ebase) and torch.equal(graphed.exp_avg, eager.exp_avg) and torch.equal(graphed.exp_avg_sq, eager.exp_avg_sq)
    assert eager.steps.tolist() == [7, 7, 7]


# ---- the trainer
OV = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10", "dropout=False"]


def _model(*extra):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    cfg = load_config(overrides=OV + ["native_optim=True"] + list(extra))
    torch.manual_seed(0)
    m = LitUnsupervisedSegmenter(27, cfg).to(DEV)
    ds = SyntheticContrastiveDataset(4, 64, 27)
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])
    return m, {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}


def test_training_step_is_the_float64_adam_step():
    m, batch = _model("native_optim_zero=False")
    facades = m.optimizers()
    fused = m._fused
    assert fused is not None and facades == fused.groups and [f.param_groups[0]["lr"] for f in facades] == [m.cfg.lr, 5e-3, 5e-3]
    before = {id(p): p.detach().cpu().numpy().copy() for f in facades for _, p in f.trainable}
    others = {n: p.detach().clone() for n, p in m.named_parameters() if id(p) not in before}
    m.training_step(batch, 0)
    torch.cuda.synchronize()
    assert fused.steps.tolist() == [1, 1, 1]
    n_moved = 0
    for f in facades:
        lr = f.param_groups[0]["lr"]
        for _, p in f.trainable:
            assert p.grad.data_ptr() == fused.bucket.flat.data_ptr() + 4 * _bucket_offset(fused, p)
            g = p.grad.detach().cpu().numpy().reshape(1, -1)                  # native_optim_zero=False: what the step used is still there
            want = adam64(before[id(p)].reshape(-1), g, lr)[0]
            got = p.detach().cpu().numpy().reshape(-1)
            bound = 2.0 ** -24 * max(np.abs(want).max(), np.abs(before[id(p)]).max()) + 2.0 ** -20 * lr
            err = np.abs(got - want).max()
            print("lr %g n %d: err %.3g bound %.3g, max|g| %.3g" % (lr, got.size, err, bound, np.abs(g).max()))
            assert err <= bound, (lr, got.size, err, bound)
            n_moved += int(np.abs(g).max() > 0)
    assert n_moved >= 5                                                        # the head and both probes received gradients
    for n, p in m.named_parameters():                                          # the frozen backbone and what no optimizer holds
        if n in others:
            assert torch.equal(p.detach(), others[n]), n

    assert fused.bucket.flat.any() and not fused.bucket_zeroed
    m.cfg.native_optim_zero = True
    zeroings = []
    fused.zero_grad = lambda: (zeroings.append(1), fused.bucket.zero_grad())
    for step in (1, 2):
        loss = m.training_step(batch, step)
        assert torch.isfinite(loss).item() and fused.bucket_zeroed
    assert len(zeroings) == 1                                                  # step 1 found stale gradients and zeroed; step 2 did not have to
    assert fused.steps.tolist() == [3, 3, 3]
    assert not fused.bucket.flat.any()
    for f in facades:
        for _, p in f.trainable:
            assert p.grad.data_ptr() == fused.bucket.flat.data_ptr() + 4 * _bucket_offset(fused, p)
    sd = facades[1].state_dict()                                               # and the facades still speak torch's layout
    adam = torch.optim.Adam(list(m.linear_probe.parameters()), lr=1.0)
    adam.load_state_dict(sd)
    assert all(float(s["step"]) == 3.0 for s in adam.state_dict()["state"].values()) and adam.param_groups[0]["lr"] == 5e-3


def _bucket_offset(fused, p):
    off = 0
    for q in fused.bucket.params:
        if q is p:
            return off
        off += q.numel()
    raise AssertionError("parameter not in the bucket")


def test_probe_reset_restarts_the_two_probe_groups():
    m, batch = _model("reset_probe_steps=1")
    m.training_step(batch, 0)
    fused = m._fused
    assert fused.steps.tolist() == [1, 1, 1]
    m.training_step(batch, 1)                                                  # global_step == 1: reset after the update
    assert fused.steps.tolist() == [2, 0, 0]
    for gi in (1, 2):
        a, b = fused._state_range[gi]
        assert not fused.exp_avg[a:b].any() and not fused.exp_avg_sq[a:b].any()
        assert fused.groups[gi].state_dict()["state"] == {}
    a, b = fused._state_range[0]
    assert fused.exp_avg[a:b].any() and fused.exp_avg_sq[a:b].any()            # the net group carries on
    loss = m.training_step(batch, 2)
    assert fused.steps.tolist() == [3, 1, 1] and torch.isfinite(loss).item()
    assert m.optimizers() == fused.groups


def test_a_cpu_models_optimizers_are_taken_over_on_the_device():
    """A checkpoint is loaded into a CPU model (torch's optimizers, whatever the flag says); on the device the facades take their state
    over."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    cfg = load_config(overrides=OV + ["native_optim=True"])
    torch.manual_seed(0)
    m = LitUnsupervisedSegmenter(27, cfg)
    adams = m.optimizers()
    assert all(isinstance(o, torch.optim.Adam) for o in adams) and m._fused is None
    for o in adams:
        for p in o.param_groups[0]["params"]:
            if p.requires_grad:
                p.grad = torch.full_like(p, 1e-3)
        o.step()
    want = [o.state_dict() for o in adams]
    m.to(DEV)
    facades = m.optimizers()
    assert m._fused is not None and facades == m._fused.groups and m._fused.steps.tolist() == [1, 1, 1]
    for f, w in zip(facades, want):
        got = f.state_dict()
        assert sorted(got["state"]) == sorted(w["state"])
        for k in w["state"]:
            assert torch.equal(got["state"][k]["exp_avg"].cpu(), w["state"][k]["exp_avg"].cpu())
            assert torch.equal(got["state"][k]["exp_avg_sq"].cpu(), w["state"][k]["exp_avg_sq"].cpu())

"""csrc/crf_loss.hip on the MI355X against the torch chain of the CRF term of LitUnsupervisedSegmenter.training_step evaluated on the
CPU in float64 through autograd (F.interpolate bilinear, F.normalize eps 1e-10, the gather, the reference's kernel and gram lines,
.mean()): the loss, the per-image means and d_code under conftest.assert_close at its defaults on the well-conditioned cases, the
shipped configuration on its own ruler, and the edge inputs (forward only, no per_image, channels-last maps, repeat launches, a
duplicated point, zero code vectors, graph capture of crf_mean_loss, one training_step with cfg.native_crf_loss off and on).

Conditioning.  With the shipped parameters the kernel k is almost diagonal: the self and duplicate pairs dominate dL/dx^ and the
normalisation's projection removes them, so at N = 1000 the gradient is 25 - 100 times smaller than the terms it is built from and
torch's own fp32 chain misses assert_close against float64.  Cases 1 - 7 and 9 - 11 are chosen so that torch's fp32 chain on the CPU uses at most
0.25 of assert_close's allowance on its worst element (tests/test_crf_loss_host.py asserts that for every case, and imports the case
table from here).  Case 8, the shipped configuration, holds d_code to max|a - e| <= 2e-6 * max|e_raw| instead, e_raw the float64
gradient of the chain with the norm detached (the un-cancelled magnitude): the random-walk estimate sqrt(N) * 2^-24 = 1.9e-6 for
N = 1000 summed terms.  Every test prints the figure it asserts on."""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHIPPED = (0.5, 0.15, 0.05, 10.0, 3.0, 0.0)                      # alpha, beta, gamma, w1, w2, shift of configs/train_config.yml
CASE8_BOUND = 2e-6


def _case(B, K, G, code, guid, grid, N, params, normalize, seed, softmax=False):
    return dict(B=B, K=K, G=G, code=code, guid=guid, grid=grid, N=N, params=params, normalize=normalize, seed=seed, softmax=softmax)


CASES = {
    1: _case(2, 70, 3, (28, 28), (224, 224), (56, 56), 1000, (0.5, 0.15, 0.05, 10.0, 3.0, 0.3), True, 7),   # the training composition
    2: _case(3, 33, 3, (7, 5), (40, 24), (14, 10), 77, SHIPPED, True, 2),            # odd K, N below a tile, non-integer ratios
    3: _case(2, 70, 3, (6, 5), (6, 5), (6, 5), 130, (0.5, 0.15, 0.05, 10.0, 3.0, 0.25), False, 3, softmax=True),   # direct, long lists
    4: _case(1, 128, 1, (9, 9), (30, 30), (18, 18), 257, (2.0, 0.5, 1.0, 1.0, 0.5, 0.1), True, 4),          # K at its limit, G = 1
    5: _case(2, 3, 4, (4, 4), (16, 16), (8, 8), 64, SHIPPED, True, 5),               # tiny K, G = 4
    6: _case(2, 27, 3, (5, 5), (5, 5), (5, 5), 1, SHIPPED, False, 6, softmax=True),  # a single point
    7: _case(2, 16, 3, (12, 12), (12, 12), (6, 6), 300, SHIPPED, True, 8),           # both maps downsampled
    8: _case(2, 70, 3, (28, 28), (224, 224), (56, 56), 1000, SHIPPED, True, 1),      # the shipped configuration
    # beyond the issue's table: the sizes at which the tap sort and the finish grid take another path
    9: _case(1, 4, 1, (8, 8), (8, 8), (16, 16), 4096, (2.0, 0.5, 1.0, 1.0, 0.5, 0.1), True, 9),     # N at its limit: 16 k keys, 128 KiB of LDS
    10: _case(1, 5, 2, (8, 8), (8, 8), (16, 16), 1500, (2.0, 0.5, 1.0, 1.0, 0.5, 0.1), True, 10),   # 8 k keys: 64 KiB, eight passes per sort step
    11: _case(17, 2, 1, (512, 512), (4, 4), (32, 32), 50, SHIPPED, False, 11),       # 17 x 16384 units > 2^18: the finish grid strides
}
WELL_CONDITIONED = (1, 2, 3, 4, 5, 6, 7, 9, 10, 11)
SMALL = (2, 3, 5, 7)


def make_inputs(case):
    """(img, code, coords) of a case, float32 / int64 on the CPU."""
    c = CASES[case] if isinstance(case, int) else case
    g = torch.Generator().manual_seed(c["seed"])
    hg, wg = c["guid"]
    img = torch.randn(c["B"], c["G"], hg, wg, generator=g)
    if hg >= 16:
        img = 2 * F.interpolate(F.avg_pool2d(img, 4), (hg, wg))          # smooth: the bilateral term is not all zero
    code = torch.randn(c["B"], c["K"], *c["code"], generator=g)
    if c["softmax"]:
        code = torch.softmax(code, 1)
    coords = torch.stack([torch.randint(0, c["grid"][0], (c["N"],), generator=g), torch.randint(0, c["grid"][1], (c["N"],), generator=g)])
    return img, code, coords


def chain(img, code, coords, grid, params, normalize, detach_norm=False):
    """The torch chain, written out: per-image means [B] of -(gram * kernel) in the dtype of the inputs."""
    alpha, beta, gamma, w1, w2, shift = params
    guidance = F.interpolate(img, grid, mode="bilinear", align_corners=False)
    clusters = F.interpolate(code, grid, mode="bilinear", align_corners=False)
    if normalize and detach_norm:
        clusters = clusters / clusters.norm(dim=1, keepdim=True).clamp_min(1e-10).detach()
    elif normalize:
        clusters = F.normalize(clusters, dim=1, eps=1e-10)
    g = guidance[:, :, coords[0], coords[1]]
    d_xy = (coords.unsqueeze(-1) - coords.unsqueeze(1)).square().sum(0).unsqueeze(0)
    d_g = (g.unsqueeze(-1) - g.unsqueeze(2)).square().sum(1)
    kernel = w1 * torch.exp(-d_xy / (2 * alpha) - d_g / (2 * beta)) + w2 * torch.exp(-d_xy / (2 * gamma)) - shift
    c = clusters[:, :, coords[0], coords[1]]
    return (-(torch.einsum("nka,nkb->nab", c, c) * kernel)).mean(dim=(1, 2))


def chain_grad(img, code, coords, c, dtype, detach_norm=False):
    """(loss, per_image, d_code) of the chain in `dtype` on the CPU, as numpy float64."""
    x = code.to(dtype).clone().requires_grad_(True)
    per_image = chain(img.to(dtype), x, coords, c["grid"], c["params"], c["normalize"], detach_norm)
    loss = per_image.mean()
    loss.backward()
    return loss.item(), per_image.detach().double().numpy(), x.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 reference of a case of the table: computed once, shared by every test, never written to."""
    img, code, coords = make_inputs(case)
    out = chain_grad(img, code, coords, CASES[case], torch.float64)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def allowance_used(actual, expected, rtol=1e-3, atol_frac=1e-4):
    """The worst element's share of assert_close's allowance: max |a - e| / (atol + rtol |e|)."""
    a, e = np.asarray(actual, dtype=np.float64).reshape(-1), np.asarray(expected, dtype=np.float64).reshape(-1)
    atol = atol_frac * float(np.mean(np.abs(e))) + 1e-12
    return float(np.max(np.abs(a - e) / (atol + rtol * np.abs(e))))


def _kernel(img, code, coords, c, **kw):
    from stego_amd import capi
    out = capi.crf_loss(img.to(DEV), code.to(DEV) if code.device != DEV else code, coords.to(DEV), c["grid"], c["params"],
                        normalize=c["normalize"], **kw)
    torch.cuda.synchronize()
    return out


def _check(k, ref, what):
    loss, per_image, d_code = k
    print("%s: allowance used: loss %.3f per_image %.3f d_code %.3f" % (
        what, allowance_used(loss.item(), ref[0]), allowance_used(per_image.cpu().numpy(), ref[1]),
        allowance_used(d_code.cpu().numpy(), ref[2])))
    assert_close(loss.item(), ref[0], what=what + " loss")
    assert_close(per_image.cpu().numpy(), ref[1], what=what + " per_image")
    assert_close(d_code.cpu().numpy(), ref[2], what=what + " d_code")


@pytest.mark.parametrize("case", WELL_CONDITIONED)
def test_parity_with_the_float64_chain(case):
    img, code, coords = make_inputs(case)
    k = _kernel(img, code, coords, CASES[case])
    assert all(torch.isfinite(t).all() for t in k)
    _check(k, reference(case), "case %d" % case)


def test_shipped_configuration_on_the_uncancelled_ruler():
    """Case 8: loss and per_image under assert_close; d_code within 2e-6 of the largest un-cancelled gradient element."""
    c = CASES[8]
    img, code, coords = make_inputs(8)
    ref = reference(8)
    e_raw = chain_grad(img, code, coords, c, torch.float64, detach_norm=True)[2]
    loss, per_image, d_code = _kernel(img, code, coords, c)
    err = float(np.abs(d_code.cpu().numpy().astype(np.float64) - ref[2]).max())
    scale = float(np.abs(e_raw).max())
    print("case 8: max|a - e| = %.3e = %.3e * max|e_raw| (max|e_raw| %.3e, max|e| %.3e); allowance used: loss %.3f per_image %.3f" % (
        err, err / scale, scale, float(np.abs(ref[2]).max()), allowance_used(loss.item(), ref[0]),
        allowance_used(per_image.cpu().numpy(), ref[1])))
    assert_close(loss.item(), ref[0], what="case 8 loss")
    assert_close(per_image.cpu().numpy(), ref[1], what="case 8 per_image")
    assert err <= CASE8_BOUND * scale, (err, scale)


@pytest.mark.parametrize("case", SMALL + (6,))
def test_forward_only_gives_the_same_loss_bits(case):
    img, code, coords = make_inputs(case)
    full = _kernel(img, code, coords, CASES[case])
    fwd = _kernel(img, code, coords, CASES[case], need_grad=False)
    assert fwd[2] is None and torch.equal(full[0], fwd[0]) and torch.equal(full[1], fwd[1])


@pytest.mark.parametrize("case", SMALL)
def test_per_image_is_optional_and_its_mean_is_the_loss(case):
    img, code, coords = make_inputs(case)
    full = _kernel(img, code, coords, CASES[case])
    without = _kernel(img, code, coords, CASES[case], want_per_image=False)
    assert without[1] is None and torch.equal(full[0], without[0]) and torch.equal(full[2], without[2])
    assert_close(full[0].item(), full[1].double().mean().item(), what="loss == mean(per_image)")


@pytest.mark.parametrize("case", SMALL)
def test_channels_last_maps_give_the_same_bits(case):
    """The head's layout: a channels-last strided view of the code in, a channels-last d_code out."""
    img, code, coords = make_inputs(case)
    dense = _kernel(img, code, coords, CASES[case])
    cl = code.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous() and cl.stride(1) == 1
    strided = _kernel(img, cl, coords, CASES[case])
    assert strided[2].stride() == cl.stride() and dense[2].is_contiguous()
    for a, e in zip(dense, strided):
        assert torch.equal(a, e)
    mixed = _kernel(img, cl, coords, CASES[case], d_code_like=dense[2])          # strided in, dense out
    assert mixed[2].is_contiguous() and torch.equal(mixed[2], dense[2])


@pytest.mark.parametrize("case", (2, 3))
def test_repeat_launches_are_bitwise_identical(case):
    img, code, coords = make_inputs(case)
    first = _kernel(img, code, coords, CASES[case])
    for _ in range(3):
        again = _kernel(img, code, coords, CASES[case])
        for a, e in zip(first, again):
            assert torch.equal(a, e)


def test_a_duplicated_point_counts_twice():
    c = CASES[3]
    img, code, coords = make_inputs(3)
    coords = coords.clone()
    coords[:, 1] = coords[:, 0]
    ref = chain_grad(img, code, coords, c, torch.float64)
    _check(_kernel(img, code, coords, c), ref, "case 3, duplicate")


def test_zero_code_vectors_in_a_block():
    """Direct mode (code at grid resolution) with the normalisation on and a block of exactly zero code vectors: torch divides their
    gradient by the eps 1e-10 without a projection.  Everything is finite; the cells outside the block pass assert_close; the cells
    inside, ten orders of magnitude larger, are compared apart with rtol 1e-3."""
    c = dict(CASES[3], normalize=True, softmax=False)
    img, code, coords = make_inputs(c)
    code[:, :, 1:3, 2:4] = 0.0
    ref = chain_grad(img, code, coords, c, torch.float64)
    loss, per_image, d_code = _kernel(img, code, coords, c)
    assert torch.isfinite(loss).all() and torch.isfinite(per_image).all() and torch.isfinite(d_code).all()
    inside = np.zeros(ref[2].shape, dtype=bool)
    inside[:, :, 1:3, 2:4] = True
    got = d_code.cpu().numpy()
    assert np.abs(ref[2][inside]).max() > 1e6 * np.abs(ref[2][~inside]).max()     # the block is touched by points
    print("zero block: allowance used: loss %.3f outside %.3f inside %.3f" % (
        allowance_used(loss.item(), ref[0]), allowance_used(got[~inside], ref[2][~inside]), allowance_used(got[inside], ref[2][inside])))
    assert_close(loss.item(), ref[0], what="loss")
    assert_close(per_image.cpu().numpy(), ref[1], what="per_image")
    assert_close(got[~inside], ref[2][~inside], what="d_code outside the zero block")
    assert_close(got[inside], ref[2][inside], rtol=1e-3, what="d_code inside the zero block")


def test_crf_mean_loss_autograd_and_graph_capture():
    """crf_mean_loss forward + backward with an upstream factor: the gradient reaches the code scaled by it, and a captured graph of
    forward + backward, replayed twice over NaN-filled outputs, reproduces the eager bits."""
    from stego_amd.crf_loss import crf_mean_loss
    c = CASES[2]
    img, code, coords = make_inputs(2)
    ref = reference(2)
    img_d, coords_d = img.to(DEV), coords.to(DEV)
    code_d = code.to(DEV).requires_grad_(True)

    def step():
        code_d.grad = None
        loss = crf_mean_loss(img_d, code_d, coords_d, c["grid"], c["params"], normalize=c["normalize"])
        (2.5 * loss).backward()
        return loss.detach().clone()

    loss = step()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and tuple(code_d.grad.shape) == tuple(code.shape)
    eager = [loss, code_d.grad.clone()]
    assert_close(loss.item(), ref[0], what="loss")
    assert_close(eager[1].cpu().numpy(), 2.5 * ref[2], what="code.grad")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = step()
        captured = [gl, code_d.grad]
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


def test_crf_mean_loss_without_a_gradient_and_the_fallback_rule():
    from stego_amd.crf_loss import _native_ok, crf_mean_loss
    c = CASES[5]
    img, code, coords = make_inputs(5)
    args = (img.to(DEV), code.to(DEV), coords.to(DEV), c["grid"], c["params"])
    assert _native_ok(*args)
    loss = crf_mean_loss(*args, normalize=True)
    assert loss.dim() == 0 and not loss.requires_grad
    assert_close(loss.item(), reference(5)[0], what="loss")
    assert not _native_ok(args[0].requires_grad_(True), *args[1:])                     # a guidance gradient: the torch chain
    assert not _native_ok(args[0].detach(), args[1].double(), *args[2:])
    assert not _native_ok(img, code, coords, c["grid"], c["params"])


def test_training_step_with_native_crf_loss_matches_the_torch_chain(monkeypatch):
    """One training_step of LitUnsupervisedSegmenter on the synthetic dataset, same weights, batch and draws, with cfg.native_crf_loss
    off and on: the fused call runs exactly when the key is on, the logged crf loss and every net parameter's .grad agree under assert_close; the probes' gradients, which do not
    depend on the term, are bitwise equal."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10",
          "dropout=False", "crf_weight=1.0", "crf_samples=200", "shift=0.1"]
    S = 5
    g = torch.Generator().manual_seed(5)
    coords1 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    coords2 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    perms = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]], device=DEV)
    points = torch.randint(0, 56, (2, 200), generator=g).to(DEV)
    models = []
    for native in (False, True):
        cfg = load_config(overrides=ov + ["native_crf_loss=%s" % native])
        assert cfg.native_crf_loss is native
        torch.manual_seed(0)
        m = LitUnsupervisedSegmenter(27, cfg)
        m.net.dropout.p = 0.0
        if models:
            m.load_state_dict(models[0][1])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m.to(DEV)
        m.contrastive_corr_loss_fn.draw = lambda of, s1, s2: (coords1, coords2, perms)
        m.crf_loss_fn.draw = lambda h, w, device: points
        models.append((m, state))
    ds = SyntheticContrastiveDataset(4, 64, 27)
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    from stego_amd import capi
    calls, native_call = [], capi.crf_loss

    def counting(*a, **kw):
        calls.append(1)
        return native_call(*a, **kw)

    monkeypatch.setattr(capi, "crf_loss", counting)
    for (m, _), expected in zip(models, (0, 1)):
        del calls[:]
        m.training_step(batch, 0)
        assert len(calls) == expected, (expected, len(calls))          # the fused call ran exactly when the key is on
    torch.cuda.synchronize()
    off, on = models[0][0], models[1][0]
    print("training_step: loss/crf off %.9g on %.9g" % (off.logged["loss/crf"].item(), on.logged["loss/crf"].item()))
    assert_close(on.logged["loss/crf"].item(), off.logged["loss/crf"].item(), what="loss/crf")
    n = 0
    for (name, pa), (_, pe) in zip(on.net.named_parameters(), off.net.named_parameters()):
        if pe.grad is not None:
            assert pa.grad is not None, name
            assert_close(pa.grad.cpu().numpy(), pe.grad.cpu().numpy(), what=name + ".grad")
            n += 1
    assert n > 0
    for name in ("linear_probe.weight", "linear_probe.bias", "cluster_probe.clusters"):
        assert torch.equal(dict(on.named_parameters())[name].grad, dict(off.named_parameters())[name].grad), name

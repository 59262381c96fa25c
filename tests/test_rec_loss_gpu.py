"""csrc/rec_loss.hip on the MI355X against the torch chain of the reconstruction term of LitUnsupervisedSegmenter.training_step
evaluated on the CPU in float64 through autograd (the 1 x 1 convolution, F.normalize eps 1e-10 of both maps, the product, .sum(1),
.mean()): the loss, d_code, d_weight and d_bias under conftest.assert_close at its defaults on the well-conditioned cases, a trained
decoder on its own ruler, and the edge inputs (forward only, single gradients, two layouts of the same maps, repeat launches, zero
feature and zero code tokens, rec_loss through autograd and graph capture, one training_step with cfg.native_rec_loss off and on).

Conditioning.  On cases 1 - 7, 9 and 10 torch's own fp32 chain on the CPU uses a small share of assert_close's allowance
(tests/test_rec_loss_host.py asserts at most 0.25 for every one of them, and imports the case table from here).  Case 8 is a trained
decoder: the cosine is almost 1, the projection cancels the gradient, d_code is about 40 times smaller than its terms and torch's fp32
itself misses assert_close.  It is held on the un-cancelled ruler max|a - e| <= bound * max|e_raw|, e_raw the float64 gradient of the
chain with the norms detached: 2 sqrt(C) 2^-24 for d_code (the two chained C-long sums, the cosine and W^T g, as random walks) and
sqrt(T) 2^-24 for d_weight and d_bias (T summed tokens).  Every test prints the figure it asserts on."""
import functools
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _case(B, K, C, hw, seed, layout="cl", init="randn", trained=False):
    return dict(B=B, K=K, C=C, hw=hw, seed=seed, layout=layout, init=init, trained=trained)


CASES = {
    1: _case(2, 70, 384, (28, 28), 1, layout="cls"),                 # the training composition: feats skip the class token
    2: _case(3, 33, 96, (7, 5), 2),                                  # odd K, C and T below or across a tile
    3: _case(1, 128, 768, (9, 9), 3),                                # K at its limit, ViT-B width
    4: _case(2, 3, 32, (4, 4), 4),                                   # tiny K and C
    5: _case(1, 27, 192, (1, 1), 5),                                 # a single token
    6: _case(2, 70, 384, (5, 5), 6, layout="nchw", init="conv"),     # the generic-stride path, nn.Conv2d's default init
    7: _case(5, 16, 65, (13, 3), 7),                                 # C not a multiple of any MFMA step, odd everything
    8: _case(2, 70, 384, (28, 28), 8, layout="cls", trained=True),   # a trained decoder: cosine ~ 1, the projection cancels
    # beyond the issue's table.  9: 142 tiles with a tail of 24 tokens: two or three tiles per token range of the d_weight launch, on
    # different waves.  10: 2056 tiles with a tail of 20 tokens: the first launch's workgroups 0 - 7 take a second tile with the grid's
    # stride (its LDS reused), and every wave of the d_weight launch adds eight or nine tiles into the same registers
    9: _case(6, 70, 96, (28, 27), 9),
    10: _case(1, 33, 65, (260, 253), 10),
}
WELL_CONDITIONED = (1, 2, 3, 4, 5, 6, 7, 9, 10)
CASE8_DCODE_BOUND = 2 * math.sqrt(384) * 2.0 ** -24                  # 2.3e-6
CASE8_DW_BOUND = math.sqrt(2 * 28 * 28) * 2.0 ** -24                 # 2.4e-6


def make_inputs(case):
    """(code [B, K, h, w], feats [B, C, h, w], weight [C, K], bias [C]) of a case: float32, contiguous, on the CPU."""
    c = CASES[case] if isinstance(case, int) else case
    g = torch.Generator().manual_seed(c["seed"])
    B, K, C, (h, w) = c["B"], c["K"], c["C"], c["hw"]
    code = torch.randn(B, K, h, w, generator=g)
    feats = torch.randn(B, C, h, w, generator=g)
    if c["init"] == "conv":
        with torch.random.fork_rng():
            torch.manual_seed(c["seed"])
            conv = nn.Conv2d(K, C, 1)
        weight, bias = conv.weight.detach().reshape(C, K).clone(), conv.bias.detach().clone()
    else:
        weight = torch.randn(C, K, generator=g) / math.sqrt(K)
        bias = 0.1 * torch.randn(C, generator=g)
    if c["trained"]:
        feats = F.conv2d(code, weight.reshape(C, K, 1, 1), bias) + 0.05 * feats
    return code, feats, weight, bias


def chain(code, feats, weight, bias, detach_norm=False):
    """The torch chain, written out, in the dtype of the inputs."""
    r = F.conv2d(code, weight.reshape(weight.shape[0], -1, 1, 1), bias)
    if detach_norm:
        rn = r / r.norm(dim=1, keepdim=True).clamp_min(1e-10).detach()
        fn = feats / feats.norm(dim=1, keepdim=True).clamp_min(1e-10)
    else:
        rn, fn = F.normalize(r, dim=1, eps=1e-10), F.normalize(feats, dim=1, eps=1e-10)
    return -(rn * fn).sum(1).mean()


def chain_grad(inputs, dtype, detach_norm=False):
    """(loss, d_code, d_weight, d_bias) of the chain in `dtype` on the CPU, as numpy float64."""
    code, feats, weight, bias = (t.to(dtype) for t in inputs)
    leaves = [t.clone().requires_grad_(True) for t in (code, weight, bias)]
    loss = chain(leaves[0], feats, leaves[1], leaves[2], detach_norm)
    loss.backward()
    return (loss.item(),) + tuple(t.grad.double().numpy() for t in leaves)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 reference of a case of the table: computed once, shared by every test, never written to."""
    out = chain_grad(make_inputs(case), torch.float64)
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw_reference(case):
    """The float64 gradients with the norms detached: the un-cancelled ruler."""
    return chain_grad(make_inputs(case), torch.float64, detach_norm=True)


def allowance_used(actual, expected, rtol=1e-3, atol_frac=1e-4):
    """The worst element's share of assert_close's allowance: max |a - e| / (atol + rtol |e|)."""
    a, e = np.asarray(actual, dtype=np.float64).reshape(-1), np.asarray(expected, dtype=np.float64).reshape(-1)
    atol = atol_frac * float(np.mean(np.abs(e))) + 1e-12
    return float(np.max(np.abs(a - e) / (atol + rtol * np.abs(e))))


def to_layout(t, layout):
    """A [B, C, h, w] map on the device in one of the layouts that occur: "cl" the contiguous [B, hw, C] map of the native head,
    "cls" the channels-last view of [B, 1 + hw, C] tokens that skips the class token, "nchw" contiguous."""
    B, C, h, w = t.shape
    if layout == "nchw":
        return t.to(DEV).contiguous()
    tok = t.permute(0, 2, 3, 1).reshape(B, h * w, C)
    if layout == "cls":
        tok = torch.cat([torch.full((B, 1, C), 7.0), tok], 1).to(DEV)[:, 1:]
    else:
        tok = tok.to(DEV).contiguous()
    return tok.reshape(B, h, w, C).permute(0, 3, 1, 2)


def _kernel(inputs, layout, **kw):
    from stego_amd import capi
    code, feats, weight, bias = inputs
    out = capi.rec_loss(to_layout(code, "nchw" if layout == "nchw" else "cl"), to_layout(feats, layout), weight.to(DEV), bias.to(DEV), **kw)
    torch.cuda.synchronize()
    return out


def _np(t):
    return t.detach().cpu().double().numpy()


def _check(k, ref, what):
    used = [allowance_used(k[0].item(), ref[0])] + [allowance_used(_np(a), e) for a, e in zip(k[1:], ref[1:])]
    print("%s: allowance used: loss %.3f d_code %.3f d_weight %.3f d_bias %.3f" % ((what,) + tuple(used)))
    for a in k:
        assert torch.isfinite(a).all(), what
    assert_close(k[0].item(), ref[0], what=what + " loss")
    for a, e, name in zip(k[1:], ref[1:], ("d_code", "d_weight", "d_bias")):
        assert tuple(a.shape) == e.shape, (name, tuple(a.shape), e.shape)
        assert_close(_np(a), e, what="%s %s" % (what, name))


@pytest.mark.parametrize("case", WELL_CONDITIONED)
def test_parity_with_the_float64_chain(case):
    c = CASES[case]
    k = _kernel(make_inputs(case), c["layout"])
    if c["layout"] == "cls":
        assert k[1].stride(1) == 1                                                      # d_code in the layout of the code
    _check(k, reference(case), "case %d" % case)


def test_trained_decoder_on_the_uncancelled_ruler():
    """Case 8: the loss under assert_close; the gradients within the stated bounds of the largest un-cancelled element."""
    k = _kernel(make_inputs(8), CASES[8]["layout"])
    ref, raw = reference(8), raw_reference(8)
    print("case 8: loss %.9g (float64 %.9g)" % (k[0].item(), ref[0]))
    assert_close(k[0].item(), ref[0], what="case 8 loss")
    for a, e, r, bound, name in zip(k[1:], ref[1:], raw[1:], (CASE8_DCODE_BOUND, CASE8_DW_BOUND, CASE8_DW_BOUND), ("d_code", "d_weight", "d_bias")):
        assert torch.isfinite(a).all(), name
        err, ruler = float(np.max(np.abs(_np(a) - e))), float(np.max(np.abs(r)))
        print("case 8 %s: max|a - e| %.3e = %.3e of max|e_raw| %.3e (bound %.3e); max|e| %.3e" % (name, err, err / ruler, ruler, bound, np.max(np.abs(e))))
        assert err <= bound * ruler, (name, err, bound * ruler)


@pytest.mark.parametrize("case", (2, 4, 7, 9, 10))
def test_forward_only_and_single_gradients_give_the_same_loss_bits(case):
    inputs, layout = make_inputs(case), CASES[case]["layout"]
    full = _kernel(inputs, layout)
    ref = reference(case)
    fwd = _kernel(inputs, layout, need_code=False, need_weight=False, need_bias=False)
    assert fwd[1] is None and fwd[2] is None and fwd[3] is None
    print("case %d: loss %.9g forward only %.9g" % (case, full[0].item(), fwd[0].item()))
    assert torch.equal(fwd[0], full[0])
    for i, name in ((1, "d_code"), (2, "d_weight"), (3, "d_bias")):
        need = dict(need_code=i == 1, need_weight=i == 2, need_bias=i == 3)
        one = _kernel(inputs, layout, **need)
        assert [j for j in (1, 2, 3) if one[j] is not None] == [i]
        assert torch.equal(one[0], full[0]), name
        assert torch.equal(one[i], full[i]), name
        assert_close(_np(one[i]), ref[i], what="case %d %s alone" % (case, name))


def test_channels_last_and_nchw_copies_agree():
    inputs = make_inputs(2)
    a, b = _kernel(inputs, "cl"), _kernel(inputs, "nchw")
    assert a[1].stride(1) == 1 and b[1].is_contiguous()
    print("case 2: loss channels-last %.9g nchw %.9g" % (a[0].item(), b[0].item()))
    for x, y, name in zip(a, b, ("loss", "d_code", "d_weight", "d_bias")):
        assert_close(_np(x), _np(y), what="channels-last against nchw: " + name)
    _check(b, reference(2), "case 2 nchw")


@pytest.mark.parametrize("case", (1, 3, 9, 10))
def test_two_launches_give_identical_bits(case):
    inputs, layout = make_inputs(case), CASES[case]["layout"]
    a, b = _kernel(inputs, layout), _kernel(inputs, layout)
    print("case %d: loss %.9g twice" % (case, a[0].item()))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("case", (2, 4))
def test_zero_feature_and_zero_code_tokens(case):
    """A token with f = 0 contributes 0 and gets a zero d_code.  With b = 0 a token with x = 0 has r = 0: it contributes 0 and, below
    eps, takes the f^ / eps gradient, ten orders of magnitude above the rest: compared apart with rtol 1e-3.  d_bias, which that token
    dominates, likewise.  Neither token produces NaN or disturbs the others."""
    code, feats, weight, bias = (t.clone() for t in make_inputs(case))
    bias.zero_()
    feats[0, :, 1, 2] = 0.0
    code[1, :, 2, 1] = 0.0
    inputs = (code, feats, weight, bias)
    ref = chain_grad(inputs, torch.float64)
    k = _kernel(inputs, CASES[case]["layout"])
    for a in k:
        assert torch.isfinite(a).all()
    d_code = _np(k[1])
    huge = np.zeros(d_code.shape, dtype=bool)
    huge[1, :, 2, 1] = True
    print("case %d: loss %.9g (float64 %.9g); max|d_code| at the f = 0 token %.3e, at the x = 0 token %.3e, elsewhere %.3e"
          % (case, k[0].item(), ref[0], np.abs(d_code[0, :, 1, 2]).max(), np.abs(d_code[huge]).max(), np.abs(d_code[~huge]).max()))
    assert_close(k[0].item(), ref[0], what="loss")
    assert (d_code[0, :, 1, 2] == 0).all()
    assert np.abs(ref[1][huge]).min() > 1e3 * np.abs(ref[1][~huge]).max()
    assert_close(d_code[~huge], ref[1][~huge], what="d_code of the other tokens")
    assert_close(d_code[huge], ref[1][huge], rtol=1e-3, what="d_code of the x = 0 token")
    assert_close(_np(k[2]), ref[2], what="d_weight")
    assert_close(_np(k[3]), ref[3], rtol=1e-3, what="d_bias")


def _decoder(case):
    code, feats, weight, bias = make_inputs(case)
    dec = nn.Conv2d(weight.shape[1], weight.shape[0], 1)
    with torch.no_grad():
        dec.weight.copy_(weight.reshape(dec.weight.shape))
        dec.bias.copy_(bias)
    return code, feats, dec.to(DEV)


def test_rec_loss_autograd_and_graph_capture():
    """rec_loss forward + backward with an upstream factor: the gradients reach the code and the decoder scaled by it, and a captured
    graph of forward + backward, replayed twice over NaN-filled outputs, reproduces the eager bits."""
    from stego_amd.rec_loss import _native_ok, rec_loss
    code, feats, dec = _decoder(2)
    ref = reference(2)
    feats_d = to_layout(feats, "cl")
    code_d = to_layout(code, "cl").detach().requires_grad_(True)
    assert _native_ok(code_d, feats_d, dec)
    leaves = (code_d, dec.weight, dec.bias)

    def step():
        for t in leaves:
            t.grad = None
        loss = rec_loss(code_d, feats_d, dec)
        (2.5 * loss).backward()
        return loss.detach().clone()

    loss = step()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and all(t.grad is not None and t.grad.shape == t.shape for t in leaves)
    eager = [loss] + [t.grad.clone() for t in leaves]
    print("rec_loss: loss %.9g (float64 %.9g)" % (loss.item(), ref[0]))
    assert_close(loss.item(), ref[0], what="loss")
    for t, e, name in zip(leaves, ref[1:], ("code.grad", "weight.grad", "bias.grad")):
        assert_close(_np(t.grad).reshape(e.shape), 2.5 * e, what=name)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = step()
        captured = [gl] + [t.grad for t in leaves]
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


def test_rec_loss_without_a_code_gradient_and_the_fallback_rule():
    from stego_amd.rec_loss import _native_ok, rec_loss, torch_rec_loss
    code, feats, dec = _decoder(4)
    code_d, feats_d = to_layout(code, "cl"), to_layout(feats, "cl")
    assert _native_ok(code_d, feats_d, dec) and not code_d.requires_grad
    loss = rec_loss(code_d, feats_d, dec)
    loss.backward()
    print("rec_loss, code.requires_grad=False: loss %.9g (float64 %.9g)" % (loss.item(), reference(4)[0]))
    assert loss.dim() == 0
    assert_close(loss.item(), reference(4)[0], what="loss")
    assert_close(_np(dec.weight.grad).reshape(reference(4)[2].shape), reference(4)[2], what="weight.grad")
    assert_close(_np(dec.bias.grad), reference(4)[3], what="bias.grad")
    assert not _native_ok(code_d, feats_d.clone().requires_grad_(True), dec)            # a feats gradient: the torch chain
    assert not _native_ok(code_d.double(), feats_d, dec)
    assert not _native_ok(code, feats, dec)
    assert not _native_ok(code_d, feats_d, nn.Conv2d(3, 32, 1, bias=False).to(DEV))
    assert not _native_ok(code_d, feats_d, nn.Conv2d(3, 32, 3, padding=1).to(DEV))
    with_grad = feats_d.clone().requires_grad_(True)
    assert_close(rec_loss(code_d, with_grad, dec).item(), torch_rec_loss(code_d, with_grad, dec).item(), what="fallback")


def _one_step(monkeypatch, rec_weight):
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10",
          "dropout=False", "rec_weight=%s" % rec_weight]
    S = 5
    g = torch.Generator().manual_seed(5)
    coords1 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    coords2 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    perms = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]], device=DEV)
    models = []
    for native in (False, True):
        cfg = load_config(overrides=ov + ["native_rec_loss=%s" % native])
        assert cfg.native_rec_loss is native
        torch.manual_seed(0)
        m = LitUnsupervisedSegmenter(27, cfg)
        m.net.dropout.p = 0.0
        if models:
            m.load_state_dict(models[0][1])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m.to(DEV)
        m.contrastive_corr_loss_fn.draw = lambda of, s1, s2: (coords1, coords2, perms)
        models.append((m, state))
    ds = SyntheticContrastiveDataset(4, 64, 27)
    batch = torch.utils.data.default_collate([ds[i] for i in range(4)])
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch.items()}
    from stego_amd import capi
    calls, native_call = [], capi.rec_loss

    def counting(*a, **kw):
        calls.append(1)
        return native_call(*a, **kw)

    monkeypatch.setattr(capi, "rec_loss", counting)
    for (m, _), expected in zip(models, (0, 1 if rec_weight > 0 else 0)):
        del calls[:]
        m.training_step(batch, 0)
        assert len(calls) == expected, (expected, len(calls))          # the fused call ran exactly when the key is on and the term is
    torch.cuda.synchronize()
    return models[0][0], models[1][0]


def test_training_step_with_native_rec_loss_matches_the_torch_chain(monkeypatch):
    """One training_step of LitUnsupervisedSegmenter on the synthetic dataset, same weights, batch and draws, with rec_weight = 1 and
    cfg.native_rec_loss off and on: the logged loss/rec and loss/total and every parameter after the step agree under assert_close."""
    off, on = _one_step(monkeypatch, 1.0)
    for key in ("loss/rec", "loss/total"):
        print("training_step: %s off %.9g on %.9g" % (key, off.logged[key].item(), on.logged[key].item()))
        assert_close(on.logged[key].item(), off.logged[key].item(), what=key)
    assert on.decoder.weight.grad is not None and on.decoder.bias.grad is not None
    n = 0
    for (name, pa), (_, pe) in zip(on.named_parameters(), off.named_parameters()):
        assert_close(_np(pa), _np(pe), what=name)
        n += 1
    assert n > 0


def test_the_flag_changes_nothing_without_the_term(monkeypatch):
    off, on = _one_step(monkeypatch, 0.0)
    assert "loss/rec" not in on.logged and "loss/rec" not in off.logged
    print("training_step, rec_weight = 0: loss/total off %.9g on %.9g" % (off.logged["loss/total"].item(), on.logged["loss/total"].item()))
    for (name, pa), (_, pe) in zip(on.named_parameters(), off.named_parameters()):
        assert torch.equal(pa, pe), name

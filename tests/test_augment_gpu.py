"""csrc/augment.hip on the MI355X against float64 on the CPU: stego_augment against tests/aug_oracle.py (the restatement of
torchvision's tensor operators of include/stego_aug.h), stego_aug_align against the torch chain of the reference's aug-alignment term
through autograd (stego_amd.augment.torch_aug_alignment).  Everything under conftest.assert_close at its defaults; the loss scalar, a
mean of cosines that cancel, within 1e-3 of the mean |cosine| term.  tests/test_augment_host.py imports the case tables from here and
asserts that fp32 on the CPU uses at most a quarter of the allowance on every case.  Every test prints the figure it asserts on."""
import functools
import itertools
import warnings

import numpy as np
import pytest
import torch

import aug_oracle
from conftest import assert_close, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NONE = 4
PERMS = list(itertools.permutations(range(4)))                              # 0 brightness, 1 contrast, 2 saturation, 3 hue


def allowance_used(actual, expected, rtol=1e-3, atol_frac=1e-4):
    """The worst element's share of assert_close's allowance: max |a - e| / (atol + rtol |e|)."""
    a, e = np.asarray(actual, dtype=np.float64).reshape(-1), np.asarray(expected, dtype=np.float64).reshape(-1)
    atol = atol_frac * float(np.mean(np.abs(e))) + 1e-12
    return float(np.max(np.abs(a - e) / (atol + rtol * np.abs(e))))


# ---- stego_augment: name -> (H, W, R, input range, seed, records as keyword sets of stego_amd.augment.make_params)
def _factors(g):
    u = torch.rand(4, generator=g).tolist()
    return (0.7 + 0.6 * u[0], 0.7 + 0.6 * u[1], 0.7 + 0.6 * u[2], -0.1 + 0.2 * u[3])


def _geometry_records(H, W):
    return [dict(), dict(flip=1),
            dict(top=0, left=0, ch=13, cw=17), dict(top=0, left=W - 9, ch=11, cw=9, flip=1),          # touching top / left / right
            dict(top=H - 11, left=0, ch=11, cw=19), dict(top=H - 7, left=W - 17, ch=7, cw=17, flip=1),  # touching bottom / left / right
            dict(top=7, left=5, ch=1, cw=1), dict(top=H - 1, left=W - 1, ch=1, cw=1, flip=1),         # 1 x 1 crops
            dict(top=3, left=4, ch=16, cw=1), dict(top=2, left=6, ch=1, cw=20, flip=1)]               # one column, one row


def _single_records():
    g = torch.Generator().manual_seed(11)
    recs = [dict(order=(op, NONE, NONE, NONE), factors=_factors(g)) for op in range(4)]
    recs += [dict(order=(NONE, op, NONE, NONE), factors=(0.7, 1.3, 0.0, 0.5), top=2, left=3, ch=25, cw=30, flip=1) for op in range(4)]
    recs += [dict(gray=1), dict(blur_sigma=0.1), dict(blur_sigma=2.0), dict(gray=1, blur_sigma=1.0, flip=1, top=1, left=2, ch=20, cw=33)]
    return recs


def _order_records(perms, seed):
    g = torch.Generator().manual_seed(seed)
    return [dict(order=o, factors=_factors(g), gray=int(i % 3 == 1), blur_sigma=(0.1, 2.0, 0.0)[i % 3], flip=i % 2,
                 top=i % 4, left=i % 5, ch=26, cw=36) for i, o in enumerate(perms)]


AUG_CASES = {
    "geometry_12": (20, 28, 12, "normal", 1, _geometry_records(20, 28)),
    "geometry_33": (20, 28, 33, "normal", 2, _geometry_records(20, 28)),            # R no multiple of a tile side or of 4
    "singles": (30, 41, 37, "unit", 3, _single_records()),                           # each operator alone
    "orders": (30, 41, 37, "unit", 4, _order_records(PERMS, 21)),                    # all 24 orders, inputs in [0, 1]
    "orders_normalised": (30, 41, 37, "normal", 5, _order_records([o for o in PERMS if o.index(0) < o.index(3)], 22)),
    "contrast_mean_224": (224, 224, 224, "unit", 6, [dict(order=(1, 0, 2, 3), factors=(1.2, 0.75, 1.1, 0.05), top=10, left=3, ch=200, cw=215),
                                                     dict(order=(0, 2, 3, 1), factors=(0.8, 1.3, 0.7, -0.1), flip=1, blur_sigma=1.3)]),
}


def aug_inputs(name):
    """(img float32 [B, 3, H, W] on the CPU, the ctypes table of records, R) of a case."""
    from stego_amd.augment import make_params, params_table
    H, W, R, kind, seed, recs = AUG_CASES[name]
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(len(recs), 3, H, W, generator=g) if kind == "normal" else torch.rand(len(recs), 3, H, W, generator=g)
    return img, params_table([make_params(H, W, **kw) for kw in recs]), R


@functools.lru_cache(maxsize=None)
def aug_reference(name):
    """The float64 oracle of a case: computed once, shared by every test, never written to."""
    img, table, R = aug_inputs(name)
    out = tuple(t.numpy() for t in aug_oracle.augment(img, table, R, torch.float64))
    for a in out:
        a.setflags(write=False)
    return out


def _augment(name, **kw):
    from stego_amd import capi
    img, table, R = aug_inputs(name)
    out = capi.augment(img.to(DEV), table, R, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(AUG_CASES))
def test_augment_matches_the_float64_oracle(name):
    img_aug, coord_aug = _augment(name)
    ref = aug_reference(name)
    assert torch.isfinite(img_aug).all() and torch.isfinite(coord_aug).all()
    print("%s: allowance used: img_aug %.3f coord_aug %.3f" % (name, allowance_used(img_aug.cpu().numpy(), ref[0]),
                                                               allowance_used(coord_aug.cpu().numpy(), ref[1])))
    assert_close(img_aug.cpu().numpy(), ref[0], what=name + " img_aug")
    assert_close(coord_aug.cpu().numpy(), ref[1], what=name + " coord_aug")
    for b in range(ref[0].shape[0]):                                        # and image by image: a small image does not hide in the mean
        assert_close(img_aug[b].cpu().numpy(), ref[0][b], what="%s img_aug[%d]" % (name, b))
        assert_close(coord_aug[b].cpu().numpy(), ref[1][b], what="%s coord_aug[%d]" % (name, b))


def test_identity_parameters_return_the_input_and_the_meshgrid():
    from stego_amd.augment import augment_batch, make_params, params_table
    img = torch.randn(2, 3, 20, 20, generator=torch.Generator().manual_seed(3)).to(DEV)
    img_aug, coord_aug = augment_batch(img, params_table([make_params(20, 20)] * 2))
    assert torch.equal(img_aug, img)
    assert_close(coord_aug.cpu().numpy(), aug_oracle.coord_image(20, 20, torch.float64).permute(1, 2, 0).expand(2, -1, -1, -1).numpy(),
                 what="coord_aug")


def test_augment_takes_a_channels_last_image():
    img, table, R = aug_inputs("orders")
    from stego_amd import capi
    dense = capi.augment(img.to(DEV), table, R)
    cl = img.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous()
    for a, e in zip(capi.augment(cl, table, R), dense):
        assert torch.equal(a, e)


@pytest.mark.parametrize("name", ["orders", "geometry_12"])                 # scalar and 16-byte stores
def test_augment_repeat_launches_are_bitwise_identical(name):
    first = _augment(name)
    for _ in range(3):
        for a, e in zip(_augment(name), first):
            assert torch.equal(a, e)


def test_augment_inside_a_captured_graph():
    """One call captured (the record table uploaded before the capture), replayed twice over NaN-filled outputs: the eager bits."""
    from stego_amd import capi
    img, table, R = aug_inputs("orders")
    img_d = img.to(DEV)
    dev_table = capi.aug_table(table, DEV)
    eager = capi.augment(img_d, table, R, table=dev_table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        capi.augment(img_d, table, R, table=dev_table)                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = capi.augment(img_d, table, R, table=dev_table)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


def test_drawn_parameters_run_and_match_the_oracle():
    from stego_amd.augment import augment_batch, draw_aug_params
    g = torch.Generator().manual_seed(8)
    img = torch.randn(6, 3, 32, 32, generator=g)
    table = draw_aug_params(6, 32, 32, 32, torch.Generator().manual_seed(9))
    img_aug, coord_aug = augment_batch(img.to(DEV), table)
    ref = aug_oracle.augment(img, table, 32, torch.float64)
    print("drawn: allowance used: img_aug %.3f coord_aug %.3f" % (allowance_used(img_aug.cpu().numpy(), ref[0].numpy()),
                                                                  allowance_used(coord_aug.cpu().numpy(), ref[1].numpy())))
    assert_close(img_aug.cpu().numpy(), ref[0].numpy(), what="img_aug")
    assert_close(coord_aug.cpu().numpy(), ref[1].numpy(), what="coord_aug")


# ---- stego_aug_align: case -> (B, K, (h, w), S, side of coord, seed)
LOSS_CASES = {
    1: (2, 70, (28, 28), 28, 224, 1),           # the training shape
    2: (3, 33, (7, 5), 6, 48, 2),               # odd K, a code that is not square
    3: (1, 128, (9, 9), 9, 9, 3),               # K at its limit; resize weights exactly 1, 0
    4: (2, 3, (4, 4), 4, 8, 4),                 # tiny K
    5: (2, 16, (5, 5), 12, 12, 5),              # more pixels than cells
}
GOLDEN_CASES = (4, 5)
LOSS_BOUND = 1e-3                               # of the mean |cosine| term


def loss_inputs(case):
    """(code, code_aug, coord) float32 on the CPU: normal codes, coordinates uniform in [-1.2, 1.2] (the border clamp is exercised)."""
    B, K, (h, w), S, Rc, seed = LOSS_CASES[case]
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, K, h, w, generator=g), torch.randn(B, K, S, S, generator=g), torch.rand(B, Rc, Rc, 2, generator=g) * 2.4 - 1.2)


def chain_grad(code, code_aug, coord, dtype):
    """(loss, d_code, d_code_aug, mean |cosine term|) of the torch chain in `dtype` on the CPU, as float / numpy float64."""
    import torch.nn.functional as F
    from stego_amd.augment import torch_aug_alignment
    x, y = code.to(dtype).clone().requires_grad_(True), code_aug.to(dtype).clone().requires_grad_(True)
    loss = torch_aug_alignment(x, y, coord.to(dtype))
    loss.backward()
    with torch.no_grad():
        ds = F.interpolate(coord.to(dtype).permute(0, 3, 1, 2), y.shape[2], mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        a = F.grid_sample(x, ds.permute(0, 2, 1, 3), padding_mode="border", align_corners=True)
        scale = (F.normalize(a, dim=1, eps=1e-10) * F.normalize(y, dim=1, eps=1e-10)).sum(1).abs().mean().item()
    return loss.item(), x.grad.double().numpy(), y.grad.double().numpy(), scale


@functools.lru_cache(maxsize=None)
def loss_reference(case):
    out = chain_grad(*loss_inputs(case), torch.float64)
    for a in out[1:3]:
        a.setflags(write=False)
    return out


def _align(code, code_aug, coord, **kw):
    from stego_amd import capi
    out = capi.aug_align(code.to(DEV) if code.device != DEV else code, code_aug.to(DEV) if code_aug.device != DEV else code_aug,
                         coord.to(DEV), **kw)
    torch.cuda.synchronize()
    return out


def _check_loss(k, ref, what):
    loss, d_code, d_code_aug = k
    err = abs(loss.item() - ref[0])
    print("%s: |loss - e| = %.3e = %.3e * mean|term| (bound %.0e); allowance used: d_code %.3f d_code_aug %.3f" % (
        what, err, err / ref[3], LOSS_BOUND, allowance_used(d_code.cpu().numpy(), ref[1]), allowance_used(d_code_aug.cpu().numpy(), ref[2])))
    assert err <= LOSS_BOUND * ref[3], (loss.item(), ref[0], ref[3])
    assert_close(d_code.cpu().numpy(), ref[1], what=what + " d_code")
    assert_close(d_code_aug.cpu().numpy(), ref[2], what=what + " d_code_aug")


@pytest.mark.parametrize("case", sorted(LOSS_CASES))
def test_aug_align_matches_the_float64_chain(case):
    k = _align(*loss_inputs(case))
    assert all(torch.isfinite(t).all() for t in k)
    _check_loss(k, loss_reference(case), "case %d" % case)


@pytest.mark.parametrize("case", (2, 5))
def test_aug_align_channels_last_codes_give_the_same_bits(case):
    code, code_aug, coord = loss_inputs(case)
    dense = _align(code, code_aug, coord)
    cl = [t.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (code, code_aug)]
    assert not cl[0].is_contiguous() and cl[0].stride(1) == 1
    strided = _align(cl[0], cl[1], coord)
    assert strided[1].stride() == cl[0].stride() and strided[2].stride() == cl[1].stride()
    for a, e in zip(strided, dense):
        assert torch.equal(a, e)
    _check_loss(strided, loss_reference(case), "case %d, channels last" % case)


def test_aug_align_zero_vectors_take_the_eps_branch():
    """A zero code_aug vector and a sampled vector that is exactly zero (a zero block of code under one coordinate): torch divides their
    gradients by the eps 1e-10 without a projection.  Everything is finite; the elements outside pass assert_close, the ones inside,
    ten orders of magnitude larger, are compared apart with rtol 1e-3."""
    code, code_aug, coord = loss_inputs(5)
    code[:, :, 0:2, 0:2] = 0.0
    coord[:, 3, 4, :] = -0.9                                 # (S = side of coord: the resize is the identity) inside the zero block
    code_aug[:, :, 7, 2] = 0.0
    ref = chain_grad(code, code_aug, coord, torch.float64)
    k = _align(code, code_aug, coord)
    assert all(torch.isfinite(t).all() for t in k)
    in_code = np.zeros(ref[1].shape, dtype=bool)
    in_code[:, :, 0:2, 0:2] = True
    in_aug = np.zeros(ref[2].shape, dtype=bool)
    in_aug[:, :, 7, 2] = True
    assert np.abs(ref[1][in_code]).max() > 1e6 * np.abs(ref[1][~in_code]).max() and np.abs(ref[2][in_aug]).max() > 1e6 * np.abs(ref[2][~in_aug]).max()
    got_code, got_aug = k[1].cpu().numpy(), k[2].cpu().numpy()
    err = abs(k[0].item() - ref[0])
    print("zero vectors: |loss - e| = %.3e * mean|term|; allowance used: d_code outside %.3f inside %.3f, d_code_aug outside %.3f inside %.3f" % (
        err / ref[3], allowance_used(got_code[~in_code], ref[1][~in_code]), allowance_used(got_code[in_code], ref[1][in_code]),
        allowance_used(got_aug[~in_aug], ref[2][~in_aug]), allowance_used(got_aug[in_aug], ref[2][in_aug])))
    assert err <= LOSS_BOUND * ref[3]
    assert_close(got_code[~in_code], ref[1][~in_code], what="d_code outside the zero block")
    assert_close(got_code[in_code], ref[1][in_code], what="d_code inside the zero block")
    assert_close(got_aug[~in_aug], ref[2][~in_aug], what="d_code_aug outside the zero pixel")
    assert_close(got_aug[in_aug], ref[2][in_aug], what="d_code_aug at the zero pixel")


@pytest.mark.parametrize("case", (2, 5))
def test_aug_align_every_coordinate_at_one_point(case):
    """One long tap list: every pixel samples the same four cells."""
    code, code_aug, coord = loss_inputs(case)
    coord[..., 0], coord[..., 1] = 0.3, -0.45
    ref = chain_grad(code, code_aug, coord, torch.float64)
    assert (np.abs(ref[1]).reshape(ref[1].shape[0], ref[1].shape[1], -1).max(1) > 0).sum() == 4 * ref[1].shape[0]
    _check_loss(_align(code, code_aug, coord), ref, "case %d, one point" % case)


@pytest.mark.parametrize("case", (2, 4, 5))
def test_aug_align_forward_only_and_single_gradients_give_the_same_bits(case):
    args = loss_inputs(case)
    full = _align(*args)
    for need_code, need_code_aug in ((False, False), (True, False), (False, True)):
        part = _align(*args, need_code=need_code, need_code_aug=need_code_aug)
        assert torch.equal(part[0], full[0])
        assert (part[1] is None) is (not need_code) and (part[2] is None) is (not need_code_aug)
        assert part[1] is None or torch.equal(part[1], full[1])
        assert part[2] is None or torch.equal(part[2], full[2])


@pytest.mark.parametrize("case", (1, 2))
def test_aug_align_repeat_launches_are_bitwise_identical(case):
    args = loss_inputs(case)
    first = _align(*args)
    for _ in range(3):
        for a, e in zip(_align(*args), first):
            assert torch.equal(a, e)


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_aug_align_golden_cases(case):
    """The inputs, the float64 loss and both gradients that the reference's own sample / norm gave (tools/make_aug_golden.py)."""
    g = load_golden("aug_align_small")
    p = "c%d_" % case
    code, code_aug, coord = (torch.from_numpy(g[p + n]) for n in ("code", "code_aug", "coord"))
    for a, e in zip((code, code_aug, coord), loss_inputs(case)):
        assert torch.equal(a, e)
    _check_loss(_align(code, code_aug, coord), (float(g[p + "loss"]), g[p + "d_code"], g[p + "d_code_aug"], float(g[p + "scale"])),
                "golden case %d" % case)


def test_aug_alignment_loss_autograd_and_graph_capture():
    """aug_alignment_loss forward + backward with an upstream factor: both gradients arrive scaled by it, and a captured graph of
    forward + backward, replayed twice over NaN-filled outputs, reproduces the eager bits."""
    from stego_amd.augment import _native_ok, aug_alignment_loss
    code, code_aug, coord = loss_inputs(2)
    ref = loss_reference(2)
    x, y, c = code.to(DEV).requires_grad_(True), code_aug.to(DEV).requires_grad_(True), coord.to(DEV)
    assert _native_ok(x, y, c) and not _native_ok(code, code_aug, coord) and not _native_ok(x.double(), y, c)

    def step():
        x.grad = y.grad = None
        loss = aug_alignment_loss(x, y, c)
        (2.5 * loss).backward()
        return loss.detach().clone()

    loss = step()
    torch.cuda.synchronize()
    assert loss.dim() == 0 and abs(loss.item() - ref[0]) <= LOSS_BOUND * ref[3]
    eager = [loss, x.grad.clone(), y.grad.clone()]
    assert_close(eager[1].cpu().numpy(), 2.5 * ref[1], what="code.grad")
    assert_close(eager[2].cpu().numpy(), 2.5 * ref[2], what="code_aug.grad")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = step()
        captured = [gl, x.grad, y.grad]
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


def test_training_step_with_native_aug_matches_the_torch_chain(monkeypatch):
    """One training_step of LitUnsupervisedSegmenter on the synthetic dataset with aug_alignment_weight = 0.5, same weights, batch,
    draws and the same img_aug / coord_aug, with cfg.native_aug off and on: the fused call runs exactly when the key is on, the logged
    loss/aug_alignment agrees and the step's loss is finite.  A third step, on a batch without the two keys, makes the view itself."""
    from stego_amd import capi
    from stego_amd.augment import augment_batch, draw_aug_params
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10",
          "dropout=False", "aug_alignment_weight=0.5"]
    S = 5
    g = torch.Generator().manual_seed(5)
    coords1 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    coords2 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    perms = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]], device=DEV)
    models = []
    for native in (False, True):
        cfg = load_config(overrides=ov + ["native_aug=%s" % native])
        assert cfg.native_aug is native
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
    bare = dict(batch)
    batch["img_aug"], batch["coord_aug"] = augment_batch(batch["img"], draw_aug_params(4, 64, 64, 64, torch.Generator().manual_seed(6)))
    calls, native_call = [], capi.aug_align

    def counting(*a, **kw):
        calls.append(1)
        return native_call(*a, **kw)

    monkeypatch.setattr(capi, "aug_align", counting)
    losses = []
    for (m, _), expected in zip(models, (0, 1)):
        del calls[:]
        losses.append(m.training_step(batch, 0))
        assert len(calls) == expected, (expected, len(calls))
    torch.cuda.synchronize()
    off, on = models[0][0], models[1][0]
    print("training_step: loss/aug_alignment off %.9g on %.9g; loss off %.9g on %.9g" % (
        off.logged["loss/aug_alignment"].item(), on.logged["loss/aug_alignment"].item(), losses[0].item(), losses[1].item()))
    assert_close(on.logged["loss/aug_alignment"].item(), off.logged["loss/aug_alignment"].item(), what="loss/aug_alignment")
    assert all(torch.isfinite(v).item() for v in losses)
    n = 0
    for (name, pa), (_, pe) in zip(on.net.named_parameters(), off.net.named_parameters()):
        if pe.grad is not None:
            assert pa.grad is not None and torch.isfinite(pa.grad).all(), name
            n += 1
    assert n > 0
    loss = on.training_step(bare, 1)                                        # no img_aug in the batch: the step makes the view
    torch.cuda.synchronize()
    assert "img_aug" in bare and tuple(bare["coord_aug"].shape) == (4, 64, 64, 2) and torch.isfinite(loss).item()
    assert on.augmenter().last_params is not None and len(on.augmenter().last_params) == 4


# ---- the loader and the trainer on the toy cropped tree of tests/golden/cropped_ref (ten 16 x 12 five-crops)
def _toy_tree(root, res):
    import os
    import shutil
    from conftest import GOLDEN
    from stego_amd import data as D
    from stego_amd.precompute_knns import nns_filename, save_nns
    dst = D.crop_dir(str(root), "cocostuff27", "five", 0.5)
    shutil.copytree(os.path.join(GOLDEN, "cropped_ref", "cropped", "toyset_five_crop_0.5"), dst)
    n = len(os.listdir(os.path.join(dst, "img", "train")))
    rng = np.random.default_rng(0)
    nns = np.stack([np.concatenate([[i], rng.permutation(np.delete(np.arange(n), i))[:8]]) for i in range(n)]).astype(np.int64)
    os.makedirs(os.path.join(str(root), "nns"))
    save_nns(os.path.join(str(root), "nns", nns_filename("vit_tiny", "cocostuff27", "train", "five", res)), nns)
    return n, nns


def test_device_loader_yields_the_augmented_view_of_its_anchors(tmp_path):
    from stego_amd import device_data as DD
    n, nns = _toy_tree(tmp_path, 32)
    store = DD.DeviceImageStore(str(tmp_path), "cocostuff27", "five", 0.5, "train", device=DEV)
    plain = DD.DeviceContrastiveLoader(store, nns, batch_size=4, res=32, seed=3)
    loaders = [DD.DeviceContrastiveLoader(store, nns, batch_size=4, res=32, seed=3, aug=True) for _ in range(2)]
    assert plain.last_aug_params is None          # (plain is iterated once, below: an iteration advances its epoch and its draws)
    for a, b, c in zip(loaders[0], loaders[1], plain):
        assert "img_aug" not in c and set(a) == set(c) | {"img_aug", "coord_aug"}
        for k in c:
            assert torch.equal(a[k], c[k]), k                                # the other keys do not change
        assert torch.equal(a["img_aug"], b["img_aug"]) and torch.equal(a["coord_aug"], b["coord_aug"])      # (seed, rank) decide
        assert tuple(a["img_aug"].shape) == (4, 3, 32, 32) and tuple(a["coord_aug"].shape) == (4, 32, 32, 2)
        table = loaders[0].last_aug_params
        assert len(table) == 4 and bytes(table) == bytes(loaders[1].last_aug_params)
        ref = aug_oracle.augment(a["img"], table, 32, torch.float64)
        assert_close(a["img_aug"].cpu().numpy(), ref[0].numpy(), what="img_aug")
        assert_close(a["coord_aug"].cpu().numpy(), ref[1].numpy(), what="coord_aug")


def test_my_app_trains_on_the_toy_tree_with_native_aug(tmp_path, capsys):
    import math
    from stego_amd import train_segmentation
    from stego_amd.train_segmentation import load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    _toy_tree(tmp_path, 64)
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "num_workers=0", "dim=16", "max_steps=3", "val_freq=100",
          "scalar_log_freq=1", "pretrained_weights=~", "pytorch_data_dir=%s" % tmp_path, "output_root=%s" % tmp_path,
          "aug_alignment_weight=0.5"]
    with pytest.raises(ValueError, match="native_aug"):
        train_segmentation.my_app(load_config(overrides=ov))
    losses = train_segmentation.my_app(load_config(overrides=ov + ["native_aug=True"]))
    assert "training data: device store (10 crops" in capsys.readouterr().out
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)
    # ... and on the synthetic path, where training_step makes the view itself
    losses = train_segmentation.my_app(load_config(overrides=[o for o in ov if not o.startswith("pytorch_data_dir")] +
                                                   ["pytorch_data_dir=~", "native_aug=True"]))
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses)

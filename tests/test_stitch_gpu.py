"""csrc/stitch_probe.hip on the MI355X: with one window over every pixel the stitched canvas is the probe head's output bit for bit;
with overlapping windows it meets the float64 oracle (tests/stitch_oracle.py) at the probe head's bar; the three output kinds agree
with each other and repeat bit for bit; the window gather is an exact copy; segment_large() and the demo's full_res run on top."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import stitch_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAR = 1e-4            # the probe head's bar on log-probabilities: a convex blend of logits that each meet it
GAP = 1e-4            # labels are compared where the oracle's two best log-probabilities are further apart than this
MAX_EXCLUDED = 0.01   # ... which may leave out at most this share of the pixels


def _inputs(T, K, hc, wc, n_lin, n_clu, seed):
    """Gaussian codes, lw ~ N(0, 1 / K), unit centroids - on the device."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(T, K, hc, wc, generator=g)
    flip = torch.randn(T, K, hc, wc, generator=g)
    lw = torch.randn(n_lin, K, generator=g) / K ** 0.5
    lb = torch.randn(n_lin, generator=g) * 0.1
    cent = F.normalize(torch.randn(n_clu, K, generator=g), dim=1)
    return [t.to(DEV) for t in (code, flip, lw, lb, cent)]


def _windows(H, W, win, stride):
    from stego_amd.segment import window_origins
    return [(oy, ox) for oy in window_origins(H, win, stride) for ox in window_origins(W, win, stride)]


def _stitch(code, flip, lw, lb, cent, size, win, stride, lin="log_probs", clu="log_probs"):
    from stego_amd import capi
    return capi.stitch_probe(code, flip, lw, lb, cent, size, win, stride, lin, clu, 2.0)


# ---- 1. single cover: the probe head, bitwise
SINGLE = [(48, 3, 96, 144), (40, 5, 80, 80), (48, 3, 48, 48)]         # win, code side, H, W; stride = win


@pytest.mark.parametrize("flip", [True, False], ids=["flip", "noflip"])
@pytest.mark.parametrize("K,n_lin,n_clu", [(70, 27, 29), (16, 3, 3), (128, 64, 64), (32, 12, 16)])        # 32, 8, 64 and 16 label slots
@pytest.mark.parametrize("layout", SINGLE, ids=lambda l: "win%d_code%d_%dx%d" % l)
def test_single_cover_is_the_probe_head_bitwise(layout, K, n_lin, n_clu, flip):
    from stego_amd import capi
    win, hc, H, W = layout
    wins = _windows(H, W, win, win)
    code, fl, lw, lb, cent = _inputs(len(wins), K, hc, hc, n_lin, n_clu, seed=K + H + W)
    fl = fl if flip else None
    for kind in ("log_probs", "probs", "argmax"):
        head = capi.probe_head(code, fl, lw, lb, cent, (win, win), kind, kind, 2.0)
        got = _stitch(code, fl, lw, lb, cent, (H, W), win, win, kind, kind)
        for h, g in zip(head, got):
            want = torch.empty_like(g)
            for t, (oy, ox) in enumerate(wins):
                want[..., oy:oy + win, ox:ox + win] = h[t]
            assert g.dtype == h.dtype and torch.equal(g, want), (kind, layout)


def test_single_cover_channels_last_code():
    """The head's channels-last views go in without a copy."""
    from stego_amd import capi
    win, hc, H, W = SINGLE[0]
    wins = _windows(H, W, win, win)
    code, fl, lw, lb, cent = _inputs(len(wins), 70, hc, hc, 27, 29, seed=11)
    cl, fcl = [t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (code, fl)]
    assert not cl.is_contiguous()
    for kind in ("log_probs", "argmax"):
        head = capi.probe_head(code, fl, lw, lb, cent, (win, win), kind, kind, 2.0)
        got = _stitch(cl, fcl, lw, lb, cent, (H, W), win, win, kind, kind)
        for h, g in zip(head, got):
            for t, (oy, ox) in enumerate(wins):
                assert torch.equal(g[..., oy:oy + win, ox:ox + win], h[t]), (kind, t)


# ---- 2. overlap: the float64 oracle
OVERLAP = [  # win, code side, stride, H, W, K, n_lin, n_clu
    (48, 3, 24, 101, 77, 70, 27, 29),       # the shifted last window overlaps on both axes: cover reaches 9
    (48, 3, 32, 100, 130, 70, 27, 29),
    (40, 5, 40, 100, 93, 70, 27, 29),
    (48, 3, 48, 100, 96, 70, 27, 29),
    (48, 3, 24, 101, 77, 128, 64, 64),      # 64 label slots: one launch per probe
    (48, 3, 24, 101, 77, 16, 3, 3),         # 8 label slots
    (48, 3, 24, 101, 77, 32, 12, 16),       # 16 label slots: stitch_probe_kernel<16, true, true, PASS_ALL> (27 + 29 above: 32)
]
_cache = {}


def _overlap(case):
    """Kernel outputs of all three kinds and the oracle's log-probabilities for `case`, computed once."""
    if case not in _cache:
        win, hc, stride, H, W, K, n_lin, n_clu = case
        T = len(_windows(H, W, win, stride))
        ins = _inputs(T, K, hc, hc, n_lin, n_clu, seed=sum(case))
        out = {kind: _stitch(*ins, (H, W), win, stride, kind, kind) for kind in ("log_probs", "probs", "argmax")}
        torch.cuda.synchronize()
        _cache[case] = (ins, out, O.stitch_log_probs(*ins, (H, W), win, stride))
    return _cache[case]


def _labels_agree(name, got, oracle_lp):
    """`got` int64 [H, W] equals the oracle's argmax wherever its top-2 gap exceeds GAP; that rule leaves out at most 1 %."""
    gap = O.top2_gap(oracle_lp)
    decided = gap > GAP
    excluded = 1.0 - decided.double().mean().item()
    wrong = int(((got.cpu() != oracle_lp.argmax(0)) & decided).sum())
    print("%s: excluded share %.5f, mismatches among the rest %d" % (name, excluded, wrong))
    assert excluded <= MAX_EXCLUDED, (name, excluded)
    assert wrong == 0, (name, wrong)


@pytest.mark.parametrize("case", OVERLAP, ids=lambda c: "win%d_code%d_s%d_%dx%d_K%d_n%d+%d" % c)
def test_overlap_against_the_float64_oracle(case):
    win, hc, stride, H, W, K, n_lin, n_clu = case
    ins, out, oracle = _overlap(case)
    if case == OVERLAP[0]:
        assert int(O.cover(H, W, win, stride).max()) == 9
    for name, n, lp, pr, am, olp in zip(("linear", "cluster"), (n_lin, n_clu), out["log_probs"], out["probs"], out["argmax"], oracle):
        assert lp.shape == (n, H, W) and lp.dtype == torch.float32 and pr.shape == (n, H, W) and pr.dtype == torch.float32
        assert am.shape == (H, W) and am.dtype == torch.int64
        assert torch.isfinite(lp).all() and torch.isfinite(pr).all(), name
        err = (lp.double().cpu() - olp).abs().max().item()
        err_p = (lp.exp() - pr).abs().max().item()
        print("%s: max |log_probs - oracle| %.3e, max |exp(log_probs) - probs| %.3e" % (name, err, err_p))
        assert err <= BAR, (name, err)
        assert err_p <= 1e-6, (name, err_p)
        assert torch.equal(am, lp.argmax(0)), name
        _labels_agree(name, am, olp)


def test_repeat_launches_are_bitwise_equal():
    case = OVERLAP[0]
    win, hc, stride, H, W = case[:5]
    ins, out, _ = _overlap(case)
    for kind in ("log_probs", "probs", "argmax"):
        again = _stitch(*ins, (H, W), win, stride, kind, kind)
        assert torch.equal(again[0], out[kind][0]) and torch.equal(again[1], out[kind][1]), kind


def test_skipped_probe_reads_nothing_of_it():
    """A skipped probe's weights and output may be NULL; the other probe's result does not change."""
    from stego_amd import capi
    for case in (OVERLAP[0], OVERLAP[4]):
        win, hc, stride, H, W, K, n_lin, n_clu = case
        (code, fl, lw, lb, cent), out, _ = _overlap(case)
        lin, none = _stitch(code, fl, lw, lb, None, (H, W), win, stride, "log_probs", None)
        assert none is None and torch.equal(lin, out["log_probs"][0])
        none, clu = _stitch(code, fl, None, None, cent, (H, W), win, stride, None, "argmax")
        assert none is None and torch.equal(clu, out["argmax"][1])
        desc = capi.stitch_desc(H, W, win, stride, code.shape[0], K, hc, hc, 0, n_clu, capi.PROBE_SKIP, capi.PROBE_PROBS, 2.0)
        probs = torch.empty(n_clu, H, W, device=DEV)
        assert capi.stitch_probe_raw(desc, capi._map(code), capi._map(fl), None, None, cent, None, probs) == 0
        assert torch.equal(probs, out["probs"][1])


# ---- 3. the window gather
def test_window_gather_copies_every_window():
    from stego_amd import capi
    H, W, win, stride = 101, 77, 48, 24
    g = torch.Generator().manual_seed(3)
    img = torch.randn(3, H, 2 * W, generator=g).to(DEV)[:, :, ::2]            # not contiguous
    assert not img.is_contiguous()
    wins = _windows(H, W, win, stride)
    out, mirrored = capi.window_gather(img, win, stride, 0, len(wins), flip=True)
    assert out.shape == (len(wins), 3, win, win) and mirrored.shape == out.shape
    for t, (oy, ox) in enumerate(wins):
        want = img[:, oy:oy + win, ox:ox + win]
        assert torch.equal(out[t], want), t
        assert torch.equal(mirrored[t], want.flip(2)), t
    assert torch.equal(mirrored, out.flip(dims=[3]))
    part = capi.window_gather(img, win, stride, 5, 4)
    assert torch.equal(part, out[5:9])
    part, part_m = capi.window_gather(img.contiguous(), win, stride, 9, 3, flip=True)
    assert torch.equal(part, out[9:12]) and torch.equal(part_m, mirrored[9:12])
    with pytest.raises(RuntimeError, match="error 125"):
        capi.window_gather(img, win, stride, 9, 4)


# ---- 4. segment_large end to end (the tiny model of tests/test_demo_gpu.py)
RES = 48


@pytest.fixture(scope="module")
def model():
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    cfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % RES, "dim=70", "dropout=False",
                                 "extra_clusters=2"])
    torch.manual_seed(1)
    return LitUnsupervisedSegmenter(27, cfg).eval().to(DEV)


def _image(H, W, seed):
    return torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_segment_large_without_overlap_is_segment_on_the_windows(model):
    from stego_amd.segment import segment, segment_large
    H, W = 96, 144
    img = _image(H, W, 4)
    lin, clu = segment_large(model, img, RES, stride=RES, run_crf=False)
    wins = _windows(H, W, RES, RES)
    assert len(wins) == 6
    stack = torch.stack([img[:, oy:oy + RES, ox:ox + RES] for oy, ox in wins])
    wl, wc = segment(model, stack, run_crf=False)
    for got, want in ((lin, wl), (clu, wc)):
        assert got.shape == (H, W) and got.dtype == torch.int64
        for t, (oy, ox) in enumerate(wins):
            assert torch.equal(got[oy:oy + RES, ox:ox + RES], want[t]), t


def test_segment_large_with_overlap_against_the_oracle(model):
    from stego_amd import capi
    from stego_amd.segment import segment_large
    H, W = 101, 77
    img = _image(H, W, 5)
    lin, clu = segment_large(model, img, RES, run_crf=False)                    # default stride: 24
    assert lin.shape == (H, W) and clu.shape == (H, W) and lin.dtype == torch.int64
    with torch.no_grad():
        wins, mirrored = capi.window_gather(img, RES, 24, 0, 12, flip=True)
        code, code_flip = model.net(wins)[1].float(), model.net(mirrored)[1].float()
        lw = model.linear_probe.weight.detach().reshape(27, 70)
        cent = F.normalize(model.cluster_probe.clusters.detach(), dim=1)
    olin, oclu = O.stitch_log_probs(code, code_flip, lw, model.linear_probe.bias.detach(), cent, (H, W), RES, 24)
    _labels_agree("linear", lin, olin)
    _labels_agree("cluster", clu, oclu)


def test_segment_large_with_the_crf_and_batches(model):
    from stego_amd.segment import segment_large
    H, W = 101, 77
    imgs = torch.stack([_image(H, W, 6), _image(H, W, 7)])
    lin, clu = segment_large(model, imgs[0], RES)
    for pred, bound in ((lin, 27), (clu, 29)):
        assert pred.shape == (H, W) and pred.dtype == torch.int64 and 0 <= int(pred.min()) and int(pred.max()) < bound
    again = segment_large(model, imgs[0], RES)
    assert torch.equal(again[0], lin) and torch.equal(again[1], clu)
    for run_crf in (True, False):
        both = segment_large(model, imgs, RES, run_crf=run_crf)
        singles = [segment_large(model, im, RES, run_crf=run_crf) for im in imgs]
        for p in (0, 1):
            assert both[p].shape == (2, H, W)
            assert torch.equal(both[p], torch.stack([s[p] for s in singles])), (run_crf, p)
    small = segment_large(model, imgs[0], RES, batch=5, run_crf=False)           # the windows in chunks of 5, 5 and 2
    assert small[0].shape == (H, W)


# ---- 5. the demo
def test_demo_full_res(tmp_path):
    from stego_amd import demo_segmentation as D
    from stego_amd.data import full_image_transform
    from stego_amd.segment import segment_large
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    mcfg = load_config(overrides=["model_type=vit_tiny", "dino_patch_size=16", "res=%d" % RES, "dim=70", "dropout=False",
                                  "extra_clusters=2"])
    torch.manual_seed(1)
    ck = tmp_path / "demo.ckpt"
    LitUnsupervisedSegmenter(27, mcfg).save_checkpoint(str(ck))
    d = tmp_path / "images"
    d.mkdir()
    rng = np.random.default_rng(2)
    Image.fromarray(rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)).save(d / "wide.jpg")
    Image.fromarray(rng.integers(0, 256, (100, 50), dtype=np.uint8), "L").save(d / "tall_gray.png")
    Image.fromarray(rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)).save(d / "small.png")
    sizes = {"wide": (60, 90), "tall_gray": (100, 50), "small": (48, 48)}

    def run(name, *extra):
        cfg = load_config(D.DEMO_CONFIG, overrides=["output_root=%s" % tmp_path, "model_path=%s" % ck, "image_dir=%s" % d,
                                                    "experiment_name=%s" % name, "res=%d" % RES, "batch_size=2", "num_workers=0"]
                          + list(extra))
        written = D.my_app(cfg)
        assert len(written) == 6
        out = os.path.join(str(tmp_path), "results", "predictions", name)
        return {(sub, stem): np.asarray(Image.open(os.path.join(out, sub, stem + ".png"))) for sub in ("linear", "cluster")
                for stem in sizes}

    full = run("full", "full_res=True")
    loaded = LitUnsupervisedSegmenter.load_from_checkpoint(str(ck)).eval().to(DEV)
    tf = full_image_transform(RES)
    for stem, ext in (("wide", ".jpg"), ("tall_gray", ".png"), ("small", ".png")):
        img = tf(Image.open(d / (stem + ext)).convert("RGB")).to(DEV)
        assert tuple(img.shape[1:]) == sizes[stem]
        lin, clu = segment_large(loaded, img, RES, batch=4)
        for sub, pred in (("linear", lin), ("cluster", clu)):
            arr = full[(sub, stem)]
            assert arr.dtype == np.uint8 and arr.shape == sizes[stem], (sub, stem, arr.shape)
            assert np.array_equal(arr, pred.cpu().numpy().astype(np.uint8)), (sub, stem)

    off, plain = run("fr_off", "full_res=False", "run_crf=False"), run("fr_plain", "run_crf=False")
    for key, arr in plain.items():
        assert arr.shape == (RES, RES) and np.array_equal(arr, off[key]), key

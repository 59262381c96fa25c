"""csrc/probe_train.hip on the MI355X against the torch chain of LitUnsupervisedSegmenter.training_step evaluated on the CPU in
float64 (F.conv2d, F.interpolate bilinear, torch.where, F.cross_entropy(ignore_index=-100), ClusterLookup.forward(x, None)): both
losses, n_valid and the three parameter gradients under conftest.assert_close at its defaults, the edge inputs (strided code, images
or batches without a valid label, zero code vectors, an exact tie of two clusters), bitwise repeatability, graph capture of
probe_losses, and one training_step with cfg.native_probes off and on.

Cluster assignments must be unambiguous for a comparison of gradients to mean anything: every test asserts first that the float64
minimum gap between the two largest cosines over all pixels is >= 1e-4 (the seeds below were chosen for that on the CPU)."""
import functools
import warnings

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MIN_GAP = 1e-4


def _inputs(B, K, h, w, H, W, n_lin, n_clu, seed):
    """The generator layout of tests/test_probe_head_gpu.py::_inputs, then the labels: randint(-1, n_lin + 1), so -1 and n_lin are
    both invalid."""
    g = torch.Generator().manual_seed(seed)
    code = torch.randn(B, K, h, w, generator=g)
    torch.randn(B, K, h, w, generator=g)                       # (the flipped code of that layout: not used here)
    Wt = torch.randn(max(n_lin, 1), K, generator=g) / K ** 0.5
    b = torch.randn(max(n_lin, 1), generator=g) * 0.1
    cent = torch.randn(max(n_clu, 1), K, generator=g)
    label = torch.randint(-1, max(n_lin, 1) + 1, (B, H, W), generator=g)
    return code, label, Wt, b, cent


def _top2_gap(code, cent, skip_rows=()):
    inner = torch.einsum("bchw,nc->bnhw", F.normalize(code.double(), dim=1), F.normalize(cent.double(), dim=1))
    keep = [i for i in range(cent.shape[0]) if i not in skip_rows]
    top = inner[:, keep].topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _chain64(code, label, Wt, b, cent, lin=True, clu=True):
    """The reference: training_step's probe lines on the CPU in float64 -> (linear loss, cluster loss, n_valid, dW, db, dC)."""
    from stego_amd.featurizers import ClusterLookup
    code = code.double()
    out = [None] * 6
    if lin:
        Wp, bp = Wt.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
        logits = F.interpolate(F.conv2d(code, Wp[:, :, None, None], bp), label.shape[-2:], mode="bilinear", align_corners=False)
        valid = (label >= 0) & (label < Wt.shape[0])
        loss = F.cross_entropy(logits, torch.where(valid, label, torch.full_like(label, -100)), ignore_index=-100)
        out[0], out[2] = loss.detach(), int(valid.sum())
        if out[2]:
            loss.backward()
            out[3], out[4] = Wp.grad, bp.grad
        else:
            out[3], out[4] = torch.zeros_like(Wp), torch.zeros_like(bp)
    if clu:
        probe = ClusterLookup(cent.shape[1], cent.shape[0]).double()
        with torch.no_grad():
            probe.clusters.copy_(cent.double())
        loss, _ = probe(code, None)
        loss.backward()
        out[1], out[5] = loss.detach(), probe.clusters.grad
    return out


def _kernel(code, label, Wt, b, cent, lin=True, clu=True):
    from stego_amd import capi
    r = capi.probe_train(code.to(DEV) if code.device != DEV else code, label.to(DEV), Wt.to(DEV) if lin else None, b.to(DEV) if lin else None,
                         cent.to(DEV) if clu else None)
    torch.cuda.synchronize()
    return r


def _compare(k, ref, lin=True, clu=True, what=""):
    losses, n_valid, dW, db, dC = k
    if lin:
        assert int(n_valid.item()) == ref[2], (what, int(n_valid.item()), ref[2])
        assert_close(losses[0].item(), ref[0].item(), what=what + " linear loss")
        assert_close(dW.cpu().numpy(), ref[3].numpy(), what=what + " d_lin_w")
        assert_close(db.cpu().numpy(), ref[4].numpy(), what=what + " d_lin_b")
    if clu:
        assert_close(losses[1].item(), ref[1].item(), what=what + " cluster loss")
        assert_close(dC.cpu().numpy(), ref[5].numpy(), what=what + " d_clusters")


def _worst_rel(k, ref, lin, clu):
    """max |a - e| / (|e| + 1e-4 mean|e|) per output: the figure INTEGRATION.md quotes (printed, not asserted)."""
    out = {}
    for name, a, e, on in (("d_lin_w", k[2], ref[3], lin), ("d_lin_b", k[3], ref[4], lin), ("d_clusters", k[4], ref[5], clu)):
        if on:
            a, e = a.cpu().double(), e.double()
            out[name] = float(((a - e).abs() / (e.abs() + 1e-4 * e.abs().mean() + 1e-300)).max())
    if lin:
        out["linear"] = abs(k[0][0].item() - ref[0].item()) / abs(ref[0].item())
    if clu:
        out["cluster"] = abs(k[0][1].item() - ref[1].item()) / abs(ref[1].item())
    return out


CASES = [  # (B, K, h, w, H, W, n_lin, n_clu), seed
    ((2, 70, 12, 12, 96, 96, 27, 27), 8),          # the training ratio
    ((3, 16, 5, 7, 37, 53, 27, 27), 20),           # non-integer ratios, tile edges
    ((2, 33, 9, 11, 40, 30, 5, 7), 26),            # odd K, small n
    ((1, 128, 6, 6, 48, 48, 64, 3), 5),            # the limits
    ((2, 70, 12, 12, 8, 8, 27, 28), 13),           # downsampling
    ((2, 70, 14, 14, 112, 112, 27, 0), 1),         # the linear probe alone
    ((2, 70, 14, 14, 112, 112, 0, 27), 27),        # the cluster probe alone; the skipped slot is untouched
    ((8, 2, 1, 600, 1, 4, 5, 0), 5),               # 150x downsampling at small K: one tile's footprint has 452 columns, more than 256 threads
    ((2, 32, 15, 17, 121, 135, 12, 16), 0),        # 8 < max(n_lin, n_clu) <= 16: probe_train_kernel<16> (the rows above: <32>, <8>, <64>)
]


@functools.lru_cache(maxsize=None)
def _case(shape, seed):
    """Inputs and their float64 reference, computed once per case and shared (nobody writes to them)."""
    x = _inputs(*shape, seed)
    lin, clu = shape[6] > 0, shape[7] > 0
    return x, _chain64(*x, lin=lin, clu=clu)


@pytest.mark.parametrize("shape,seed", CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else "seed%d" % c)
def test_parity_with_the_float64_chain(shape, seed):
    (code, label, Wt, b, cent), ref = _case(shape, seed)
    lin, clu = shape[6] > 0, shape[7] > 0
    if clu:
        assert _top2_gap(code, cent).min().item() >= MIN_GAP
    if lin:
        share = ((label >= 0) & (label < shape[6])).double().mean().item()
        assert 0.6 <= share <= 0.99, share
    k = _kernel(code, label, Wt, b, cent, lin, clu)
    print("worst relative errors %s seed %d: %s" % (shape, seed, _worst_rel(k, ref, lin, clu)))
    _compare(k, ref, lin, clu, what=str(shape))
    if not lin:
        assert k[0][0].item() == 0.0 and k[2] is None and k[3] is None      # capi.probe_train zeroes the slots; the kernel left it alone
    if not clu:
        assert k[0][1].item() == 0.0 and k[4] is None


def test_skipped_probe_leaves_its_loss_slot_untouched():
    from stego_amd import capi
    shape, seed = CASES[6]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    B, K, h, w, H, W, _, n_clu = shape
    code, cent = code.to(DEV), cent.to(DEV)
    losses = torch.full((2,), 123.0, device=DEV)
    n_valid = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    dC = torch.empty(n_clu, K, device=DEV)
    desc = capi.probe_train_desc(B, K, h, w, H, W, 0, n_clu)
    n = capi.probe_train_workspace_bytes(desc)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    rc = capi.probe_train_raw(desc, capi._map(code), None, None, None, cent, losses, n_valid, None, None, dC, ws, n, capi._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert losses[0].item() == 123.0 and losses[1].item() != 123.0 and n_valid.item() == 0


def test_channels_last_strided_code_gives_the_same_bits():
    shape, seed = CASES[1]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    dense = _kernel(code, label, Wt, b, cent)
    cl = code.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # [B, K, h, w] view of channels-last memory
    assert cl.stride(1) == 1 and not cl.is_contiguous()
    strided = _kernel(cl, label, Wt, b, cent)
    for a, e in zip(dense, strided):
        assert torch.equal(a, e)


def test_one_image_without_a_valid_label():
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    label = label.clone()
    label[1] = -1
    ref = _chain64(code, label, Wt, b, cent)
    assert ref[2] == int(((label[0] >= 0) & (label[0] < shape[6])).sum())
    k = _kernel(code, label, Wt, b, cent)
    _compare(k, ref, what="image 1 invalid")
    # the other image alone gives the same linear probe numbers
    alone = _chain64(code[:1], label[:1], Wt, b, cent, clu=False)
    assert_close(k[0][0].item(), alone[0].item(), what="linear loss of image 0 alone")
    assert_close(k[2].cpu().numpy(), alone[3].numpy(), what="d_lin_w of image 0 alone")


def test_no_valid_label_at_all():
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), ref = _case(shape, seed)
    bad = torch.where(label % 2 == 0, torch.full_like(label, -1), torch.full_like(label, shape[6]))
    losses, n_valid, dW, db, dC = _kernel(code, bad, Wt, b, cent)
    assert n_valid.item() == 0 and torch.isnan(losses[0])
    assert torch.equal(dW, torch.zeros_like(dW)) and torch.equal(db, torch.zeros_like(db))
    assert_close(losses[1].item(), ref[1].item(), what="cluster loss")               # the cluster probe does not see labels
    assert_close(dC.cpu().numpy(), ref[5].numpy(), what="d_clusters")
    # without the cluster probe too: all three gradients of the call are exactly zero
    losses, n_valid, dW, db, _ = _kernel(code, bad, Wt, b, cent, clu=False)
    assert n_valid.item() == 0 and torch.isnan(losses[0]) and not dW.any() and not db.any()


def test_every_label_invalid_zeroes_all_three_gradients_with_zero_code():
    """Every label invalid and a zero code: the linear loss is NaN and all three gradients are exactly zero (a zero vector normalises
    to zero, so no cluster receives anything)."""
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    losses, n_valid, dW, db, dC = _kernel(torch.zeros_like(code), torch.full_like(label, -1), Wt, b, cent)
    assert n_valid.item() == 0 and torch.isnan(losses[0]) and losses[1].item() == 0.0
    assert not dW.any() and not db.any() and not dC.any()


def test_zero_code_vectors_in_a_block():
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    code = code.clone()
    code[0, :, 3:7, 2:9] = 0.0
    nonzero = code.abs().sum(1) > 0
    assert _top2_gap(code, cent)[nonzero].min().item() >= MIN_GAP       # (a zero vector ties every cluster at 0: both sides take the first)
    ref = _chain64(code, label, Wt, b, cent)
    k = _kernel(code, label, Wt, b, cent)
    for t in k:
        assert torch.isfinite(t.float()).all()
    _compare(k, ref, what="zero block")


def test_exact_tie_goes_to_the_first_cluster():
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    cent = cent.clone()
    cent[5] = cent[2]
    assert _top2_gap(code, cent, skip_rows=(5,)).min().item() >= MIN_GAP
    ref = _chain64(code, label, Wt, b, cent)
    assert not ref[5][5].any() and ref[5][2].any()                      # torch.argmax takes the first of the two equal cosines
    k = _kernel(code, label, Wt, b, cent)
    assert not k[4][5].any()
    assert_close(k[4][2].cpu().numpy(), ref[5][2].numpy(), what="d_clusters row 2")
    _compare(k, ref, what="tie")


def test_repeat_launches_are_bitwise_identical():
    shape, seed = CASES[0]
    (code, label, Wt, b, cent), _ = _case(shape, seed)
    first = _kernel(code, label, Wt, b, cent)
    for _ in range(3):
        again = _kernel(code, label, Wt, b, cent)
        for a, e in zip(first, again):
            assert torch.equal(a, e)


def _probes(Wt, b, cent):
    from stego_amd.featurizers import ClusterLookup
    lin = torch.nn.Conv2d(Wt.shape[1], Wt.shape[0], (1, 1))
    clu = ClusterLookup(cent.shape[1], cent.shape[0])
    with torch.no_grad():
        lin.weight.copy_(Wt[:, :, None, None])
        lin.bias.copy_(b)
        clu.clusters.copy_(cent)
    return lin.to(DEV), clu.to(DEV)


def test_probe_losses_autograd_and_graph_capture():
    """probe_losses forward + backward: the gradients reach the three parameters scaled by the upstream factors, and a captured graph
    of forward + backward, replayed twice, reproduces the eager bits."""
    from stego_amd.probe_train import probe_losses
    shape, seed = CASES[1]
    (code, label, Wt, b, cent), ref = _case(shape, seed)
    lin, clu = _probes(Wt, b, cent)
    code_d, label_d = code.to(DEV).requires_grad_(True), label.to(DEV)

    def step():
        for p in (lin.weight, lin.bias, clu.clusters):
            p.grad = None
        l, c = probe_losses(code_d, label_d, lin, clu)
        (2.0 * l + 3.0 * c).backward()
        return l.detach().clone(), c.detach().clone()

    l, c = step()
    torch.cuda.synchronize()
    assert l.dim() == 0 and c.dim() == 0 and code_d.grad is None                       # the code is detached inside
    assert tuple(lin.weight.grad.shape) == tuple(lin.weight.shape)
    eager = [l, c, lin.weight.grad.clone(), lin.bias.grad.clone(), clu.clusters.grad.clone()]
    assert_close(l.item(), ref[0].item(), what="linear loss")
    assert_close(c.item(), ref[1].item(), what="cluster loss")
    assert_close(eager[2].cpu().numpy().reshape(ref[3].shape), 2.0 * ref[3].numpy(), what="weight.grad")
    assert_close(eager[3].cpu().numpy(), 2.0 * ref[4].numpy(), what="bias.grad")
    assert_close(eager[4].cpu().numpy(), 3.0 * ref[5].numpy(), what="clusters.grad")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                         # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl, gc = step()
        captured = [gl, gc, lin.weight.grad, lin.bias.grad, clu.clusters.grad]
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, e in zip(captured, eager):
            assert torch.equal(a, e)


def test_training_step_with_native_probes_matches_the_torch_chain():
    """One training_step of LitUnsupervisedSegmenter on the synthetic dataset, same weights, batch and draws, with cfg.native_probes
    off and on: the logged probe losses and the .grad of the three probe parameters agree under assert_close, the head's gradients
    within 1e-6 (they do not depend on the probes).  .grad is compared, not the parameters after the (sign-like) first Adam step."""
    from stego_amd.train_segmentation import LitUnsupervisedSegmenter, SyntheticContrastiveDataset, load_config
    warnings.filterwarnings("ignore", message="DinoFeaturizer")
    ov = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10",
          "dropout=False"]
    S = 5
    g = torch.Generator().manual_seed(5)
    coords1 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    coords2 = (torch.rand(4, S, S, 2, generator=g) * 2 - 1).to(DEV)
    perms = torch.tensor([[1, 2, 3, 0], [2, 3, 0, 1]], device=DEV)
    models = []
    for native in (False, True):
        cfg = load_config(overrides=ov + ["native_probes=%s" % native])
        assert cfg.native_probes is native
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
    with torch.no_grad():
        code = models[0][0].net(batch["img"])[1]
    assert _top2_gap(code.cpu(), models[0][1]["cluster_probe.clusters"]).min().item() >= MIN_GAP
    for m, _ in models:
        m.training_step(batch, 0)
    torch.cuda.synchronize()
    off, on = models[0][0], models[1][0]
    for k in ("loss/linear", "loss/cluster"):
        assert_close(on.logged[k].item(), off.logged[k].item(), what=k)
    for name in ("linear_probe.weight", "linear_probe.bias", "cluster_probe.clusters"):
        a, e = dict(on.named_parameters())[name].grad, dict(off.named_parameters())[name].grad
        assert a is not None and a.shape == e.shape, name
        assert_close(a.cpu().numpy(), e.cpu().numpy(), what=name + ".grad")
    for (name, pa), (_, pe) in zip(on.net.named_parameters(), off.net.named_parameters()):
        if pe.grad is not None:
            assert (pa.grad - pe.grad).abs().max().item() <= 1e-6, name

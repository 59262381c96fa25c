"""The trainable part of one LitUnsupervisedSegmenter.training_step in float64 on the CPU, composed from the references the per-unit
suites already hold (imported, not restated):

    head                 _reference_head_fp64      tests/test_head_native.py
    correspondence term  corr_loss_forward / corr_loss_backward      oracle/corr_oracle.py
    rec term             chain                     tests/test_rec_loss_gpu.py
    crf term             chain                     tests/test_crf_loss_gpu.py
    aug-alignment term   chain_grad                tests/test_augment_gpu.py
    probes               _chain64                  tests/test_probe_train_gpu.py
    update               adam64                    tests/test_optim_gpu.py

Inputs are what the device step consumed: the maps `feats`, `feats_pos` and the feats of `img_aug` as model.net returned them (with
dropout=False they are the head's input, so no backbone is needed: the reference is the same whether the tokens came from the native
ViT, the torch module or the token cache), the batch's img (the crf term's guidance), label and coord_aug, the draws fed to both
sides, and the parameters before the step.  The two terms whose references return gradients instead of a graph (correspondence, aug
alignment) enter torch autograd as <code, d_code> products, so one backward through the float64 head gives every head gradient."""
import types

import numpy as np
import torch

from oracle import corr_oracle as O
from test_augment_gpu import chain_grad as aug_chain_grad
from test_crf_loss_gpu import chain as crf_chain
from test_head_native import _reference_head_fp64
from test_optim_gpu import adam64
from test_probe_train_gpu import MIN_GAP, _chain64, _top2_gap
from test_rec_loss_gpu import chain as rec_chain

CRF_SIZE = 56                                   # training_step resizes the guidance and the code to 56 x 56 for the crf term
PROBES = ("linear_probe.weight", "linear_probe.bias", "cluster_probe.clusters")


def trainable_names(model):
    """The trainable parameters of a LitUnsupervisedSegmenter that an optimizer owns, by name, in optimizer order."""
    names = {id(p): n for n, p in model.named_parameters()}
    return [names[id(p)] for g in model.optimizer_groups() for p in g["params"] if p.requires_grad]


def capture_feats(model):
    """A forward hook on model.net that keeps the feats of every call (img, img_pos, img_aug, in the step's order) -> (list, handle)."""
    kept = []
    handle = model.net.register_forward_hook(lambda mod, args, out: kept.append(out[0].detach().clone()))
    return kept, handle


def _head(P, proj_type):
    """What _reference_head_fp64 reads of a DinoFeaturizer, over the float64 leaves P."""
    conv = lambda prefix: types.SimpleNamespace(weight=P[prefix + ".weight"], bias=P[prefix + ".bias"])
    net = types.SimpleNamespace(proj_type=proj_type, cluster1=[conv("net.cluster1.0")])
    if proj_type == "nonlinear":
        net.cluster2 = [conv("net.cluster2.0"), None, conv("net.cluster2.2")]
    return net


def corr_cfg(cfg):
    """The oracle's configuration of the correspondence term.  The shifts are the float32 values the loss descriptor carries
    (StegoCorrDesc holds them as float): the term the step evaluated, on the device and through the backend double alike."""
    f32 = lambda x: float(np.float32(x))
    return O.CorrCfg(pointwise=bool(cfg.pointwise), zero_clamp=bool(cfg.zero_clamp), stabalize=bool(cfg.stabalize),
                     feature_samples=int(cfg.feature_samples), neg_samples=int(cfg.neg_samples), pos_intra_shift=f32(cfg.pos_intra_shift),
                     pos_inter_shift=f32(cfg.pos_inter_shift), neg_inter_shift=f32(cfg.neg_inter_shift))


def step_oracle(cfg, params, feats, feats_pos, feats_aug, img, label, coord_aug, coords1, coords2, perms, points):
    """-> dict(losses: {tag: float} with every loss/* term and loss/total, cd: {tag: float} the three cd means, grads: {name: float64
    tensor} for every name in `params`, ambiguous: bool [C] (the hidden channels of cluster2.0 whose float64 pre-activation is
    within 1e-5 of zero somewhere in the three forwards) or None for a linear head, gap: the smallest float64 top-2 cosine gap of the
    cluster probe over the pixels of the code).

    cfg: the step's configuration (use_true_labels and use_salience off, correspondence_weight > 0, dropout False).  params: {name:
    tensor} of the trainable parameters before the step.  feats* [B, C, h, w], img [B, 3, H, W], label int64 [B, H, W], coord_aug
    [B, R, R, 2] or None without the aug term, coords1 / coords2 [B, S, S, 2], perms int64 [n_neg, B], points int64 [2, N] or None
    without the crf term: torch tensors on the CPU (any float dtype; everything is evaluated in float64)."""
    assert not cfg.use_true_labels and not cfg.use_salience and not cfg.dropout and cfg.correspondence_weight > 0
    P = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in params.items()}
    f, fp = feats.detach().cpu().double(), feats_pos.detach().cpu().double()
    B, C = f.shape[:2]
    ones = [torch.ones(B, C, dtype=torch.float64)] * 3             # dropout p = 0: every channel kept with weight 1
    net = _head(P, cfg.projection_type)
    _, code, amb = _reference_head_fp64(net, f, ones)
    _, code_pos, amb_pos = _reference_head_fp64(net, fp, ones)
    ambiguous = None if amb is None else amb | amb_pos
    losses, cd = {}, {}

    # correspondence term: forward and code gradients from the numpy oracle, upstream factors = the weights of the total
    cc = corr_cfg(cfg)
    S, n_neg = cc.feature_samples, int(perms.shape[0])
    corr_in = (f.numpy(), fp.numpy(), code.detach().numpy(), code_pos.detach().numpy(), coords1.detach().cpu().double().numpy(),
               coords2.detach().cpu().double().numpy(), list(perms.cpu().numpy()), cc)
    out = O.corr_loss_forward(*corr_in)
    neg_mean = float(out.neg_inter_loss.mean()) if n_neg else 0.0
    losses["loss/pos_intra"], losses["loss/pos_inter"], losses["loss/neg_inter"] = float(out.pos_intra_loss), float(out.pos_inter_loss), neg_mean
    cd["cd/pos_intra"], cd["cd/pos_inter"] = float(out.pos_intra_cd.mean()), float(out.pos_inter_cd.mean())
    cd["cd/neg_inter"] = float(out.neg_inter_cd.mean()) if n_neg else float("nan")
    w = float(cfg.correspondence_weight)
    g_nl = np.full((n_neg * B, S, S, S, S), w * cfg.neg_inter_weight / max(n_neg * B * S ** 4, 1)) if n_neg else None
    d_code, d_code_pos = O.corr_loss_backward(*corr_in, w * cfg.pos_intra_weight, w * cfg.pos_inter_weight, g_nl)
    total = w * (cfg.pos_intra_weight * losses["loss/pos_intra"] + cfg.pos_inter_weight * losses["loss/pos_inter"]
                 + cfg.neg_inter_weight * neg_mean)
    graph = (code * torch.from_numpy(d_code)).sum() + (code_pos * torch.from_numpy(d_code_pos)).sum()

    if cfg.rec_weight > 0:
        rec = rec_chain(code, f, P["decoder.weight"], P["decoder.bias"])
        losses["loss/rec"] = rec.item()
        total += cfg.rec_weight * rec.item()
        graph = graph + cfg.rec_weight * rec

    if cfg.aug_alignment_weight > 0:
        _, code_aug, amb_aug = _reference_head_fp64(net, feats_aug.detach().cpu().double(), ones)
        ambiguous = None if ambiguous is None else ambiguous | amb_aug
        aug, d_a, d_aug, _ = aug_chain_grad(code.detach(), code_aug.detach(), coord_aug.detach().cpu(), torch.float64)
        losses["loss/aug_alignment"] = aug
        total += cfg.aug_alignment_weight * aug
        graph = graph + cfg.aug_alignment_weight * ((code * torch.from_numpy(d_a)).sum() + (code_aug * torch.from_numpy(d_aug)).sum())

    if cfg.crf_weight > 0:
        crf = crf_chain(img.detach().cpu().double(), code, points.cpu(), (CRF_SIZE, CRF_SIZE),
                        (cfg.alpha, cfg.beta, cfg.gamma, cfg.w1, cfg.w2, cfg.shift), True).mean()
        losses["loss/crf"] = crf.item()
        total += cfg.crf_weight * crf.item()
        graph = graph + cfg.crf_weight * crf

    graph.backward()
    grads = {k: v.grad for k, v in P.items() if k not in PROBES}
    assert all(g is not None for g in grads.values()), [k for k, g in grads.items() if g is None]

    # both probes train on the detached code
    Wt = P["linear_probe.weight"].detach()
    lin, clu, _, dW, db, dC = _chain64(code.detach(), label.cpu(), Wt.reshape(Wt.shape[0], -1), P["linear_probe.bias"].detach(),
                                       P["cluster_probe.clusters"].detach())
    losses["loss/linear"], losses["loss/cluster"] = lin.item(), clu.item()
    total += lin.item() + clu.item()
    losses["loss/total"] = total
    grads.update({"linear_probe.weight": dW.reshape(Wt.shape), "linear_probe.bias": db, "cluster_probe.clusters": dC})
    gap = _top2_gap(code.detach(), P["cluster_probe.clusters"].detach()).min().item()
    return dict(losses=losses, cd=cd, grads={k: grads[k].detach() for k in params}, ambiguous=ambiguous, gap=gap)


def adam_update64(before, grad, lr, steps_before, exp_avg, exp_avg_sq):
    """One float64 Adam step (adam64) of a tensor from its state before the step -> the parameter after it, flat numpy float64."""
    flat = lambda t: t.detach().cpu().numpy().reshape(-1)
    return adam64(flat(before), flat(grad).reshape(1, -1), lr, steps_before=steps_before, m=flat(exp_avg), v=flat(exp_avg_sq))[0]


# ---- the shape the per-key step tests share, with every weighted term on, and the inputs of step t (the same for both sides)
SHAPE = ["model_type=vit_tiny", "dino_patch_size=16", "res=64", "batch_size=4", "feature_samples=5", "neg_samples=2", "dim=10",
         "dropout=False"]
WEIGHTS = ["crf_weight=1.0", "crf_samples=200", "shift=0.1", "rec_weight=1.0", "aug_alignment_weight=0.5"]
B, S, RES, N_CLASSES, N_POINTS = 4, 5, 64, 27, 200
_SHIFTS = ([1, 2, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2])             # the permutations of four images without a fixed point that are cyclic shifts


def step_batch(ds, step):
    """Batch `step` of the dataset in order, wrapping around (a second pass sees the same items again): CPU tensors."""
    n_batches = len(ds) // B
    first = (step % n_batches) * B
    return torch.utils.data.default_collate([ds[i] for i in range(first, first + B)])


def step_draws(step):
    """The draws of step `step`: (coords1, coords2, perms, points, the record table of the augmented view), seeded by the step."""
    from stego_amd.augment import draw_aug_params
    g = torch.Generator().manual_seed(500 + step)
    coords1 = torch.rand(B, S, S, 2, generator=g) * 2 - 1
    coords2 = torch.rand(B, S, S, 2, generator=g) * 2 - 1
    perms = torch.tensor([_SHIFTS[step % 3], _SHIFTS[(step + 1) % 3]])
    points = torch.randint(0, CRF_SIZE, (2, N_POINTS), generator=g)
    table = draw_aug_params(B, RES, RES, RES, torch.Generator().manual_seed(600 + step))
    return coords1, coords2, perms, points, table


def feed_draws(model, coords1, coords2, perms, points):
    """Replace the two draws of the step by the given ones, on the model's device."""
    dev = model.linear_probe.weight.device
    c1, c2, pm, pt = coords1.to(dev), coords2.to(dev), perms.to(dev), points.to(dev)
    model.contrastive_corr_loss_fn.draw = lambda of, s1, s2: (c1.to(of.dtype), c2.to(of.dtype), pm)
    model.crf_loss_fn.draw = lambda h, w, device: pt

"""PL-free mirror of the reference's ``src/train_segmentation.py``: ``LitUnsupervisedSegmenter`` with the same
constructor, attributes, state-dict keys and ``training_step`` arithmetic (:53-245,373-383), a small
``Trainer`` (the reference delegates to pytorch_lightning, which is not in this image), the yaml+override
config loader (hydra is absent) and a synthetic stand-in for ``ContrastiveSegDataset`` (no datasets offline).

The correspondence loss inside ``training_step`` is the HIP path (stego_amd.modules); everything else is stock
PyTorch-ROCm.  Data parallelism: one process per GPU, batch sharded, ONE flat RCCL all-reduce of the
trainable (head + probe) gradients per step (stego_amd.ddp) - the backbone is frozen, nothing inside the loss
is synchronised.

    python -m stego_amd.train_segmentation max_steps=20 batch_size=8            # synthetic data, 1 GPU
    torchrun --standalone --nproc-per-node 8 -m stego_amd.train_segmentation max_steps=20
"""
import os
import sys
import types
from os.path import dirname, join

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

from . import ddp
from .augment import Augmenter, aug_alignment_loss, needs_torchvision
from .featurizers import ClusterLookup, ContrastiveCRFLoss, DinoFeaturizer, FeaturePyramidNet
from .modules import ContrastiveCorrelationLoss, norm, sample
from .probe_train import probe_losses, torch_probe_losses
from .rec_loss import rec_loss as native_rec_loss
from .salience import attention_salience
from .metrics import DeviceUnsupervisedMetrics, probe_confusion
from .utils import UnsupervisedMetrics, one_hot_feats, prep_args, resize


def get_class_labels(dataset_name):
    """n_classes per dataset as the reference sets them (train_segmentation.py:33-50, data.py)."""
    if dataset_name.startswith("cityscapes"):
        return 27
    if dataset_name == "cocostuff27":
        return 27
    if dataset_name == "cocostuff3":
        return 3
    if dataset_name == "potsdam":
        return 3
    raise ValueError("Unknown Dataset {}".format(dataset_name))


def load_config(path=None, overrides=()):
    """yaml defaults + `key=value` overrides -> attribute-style cfg (what hydra/OmegaConf gives the reference)."""
    path = path or join(dirname(__file__), "configs", "train_config.yml")
    with open(path) as f:
        d = yaml.safe_load(f)
    for ov in overrides:
        k, v = ov.split("=", 1)
        d[k] = yaml.safe_load(v)
    return types.SimpleNamespace(**d)


MAX_CODE_DIM = 128               # include/stego_corr.h "Limits of this build" (above 72: channels-last ViT-width maps)
MAX_FEATURE_SAMPLES = 11
MAX_FEATURE_SAMPLES_WIDE = 16    # 12 .. 16: csrc/corr_wide.hip behind the same entry points (a few launches instead of one)
MAX_CODE_DIM_WIDE = 128
MAX_CODE_DIM_ANY_PATH = 72       # above it: the single-launch forward only (its conditions are checked in __init__)


class LitUnsupervisedSegmenter(nn.Module):
    def __init__(self, n_classes, cfg):
        super().__init__()
        self.cfg = cfg
        self.n_classes = n_classes
        dim = cfg.dim if cfg.continuous else n_classes
        if cfg.arch == "feature-pyramid":           # train_segmentation.py:65-67
            from .trunks import load_model
            data_dir = os.path.join(getattr(cfg, "output_root", "."), "data")
            cut_model = load_model(cfg.model_type, data_dir, allow_random_init=getattr(cfg, "allow_random_trunk", False))
            self.net = FeaturePyramidNet(cfg.granularity, cut_model, dim, cfg.continuous)
        elif cfg.arch == "dino":
            self.net = DinoFeaturizer(dim, cfg)
        else:
            raise ValueError("Unknown arch {}".format(cfg.arch))
        self.train_cluster_probe = ClusterLookup(dim, n_classes)
        # cfg.cluster_probe_n (a stego_amd extension, absent from shipped configs and old checkpoints): the cluster count of a probe that
        # stego_amd.cluster_refit refitted; the metrics then treat what exceeds n_classes as extra clusters
        probe_n = getattr(cfg, "cluster_probe_n", None)
        cluster_extra = cfg.extra_clusters if probe_n is None else max(int(probe_n) - n_classes, 0)
        self.cluster_probe = ClusterLookup(dim, n_classes + cfg.extra_clusters if probe_n is None else int(probe_n))
        self.linear_probe = nn.Conv2d(dim, n_classes, (1, 1))
        self.decoder = nn.Conv2d(dim, self.net.n_feats, (1, 1))
        # cfg.native_metrics: the confusion matrices stay on the device and validation_step scores with one fused call (stego_amd.metrics)
        Metrics = DeviceUnsupervisedMetrics if getattr(cfg, "native_metrics", False) else UnsupervisedMetrics
        self.cluster_metrics = Metrics("test/cluster/", n_classes, cluster_extra, True)
        self.linear_metrics = Metrics("test/linear/", n_classes, 0, False)
        self.test_cluster_metrics = Metrics("final/cluster/", n_classes, cluster_extra, True)
        self.test_linear_metrics = Metrics("final/linear/", n_classes, 0, False)
        self.linear_probe_loss_fn = nn.CrossEntropyLoss()
        self.crf_loss_fn = ContrastiveCRFLoss(cfg.crf_samples, cfg.alpha, cfg.beta, cfg.gamma, cfg.w1, cfg.w2, cfg.shift)
        self.contrastive_corr_loss_fn = ContrastiveCorrelationLoss(cfg)
        # limits of this build of libstego_corr (include/stego_corr.h): fail here, with the cfg keys named, not with
        # STEGO_ERR_UNSUPPORTED inside the first training_step
        if cfg.correspondence_weight > 0:
            if dim > MAX_CODE_DIM:
                import warnings
                warnings.warn("cfg.dim=%d: the fused loss kernels cover code dimensions up to %d (train_config.yml:39 ships 70; "
                              "include/stego_corr.h); this configuration runs on ContrastiveCorrelationLoss.generic_forward: same "
                              "results, several times slower" % (dim, MAX_CODE_DIM))
            if cfg.feature_samples > MAX_FEATURE_SAMPLES_WIDE or (cfg.feature_samples > MAX_FEATURE_SAMPLES and dim > MAX_CODE_DIM_WIDE):
                import warnings
                warnings.warn("cfg.feature_samples=%d, cfg.dim=%d: the single-launch loss kernels cover S <= %d (train_config.yml:51 ships 11), the "
                              "multi-launch kernels S <= %d with dim <= %d; this configuration runs on ContrastiveCorrelationLoss.generic_forward "
                              "(the same native samplers and correlation kernels composed in Python): same results, slower and host-bound"
                              % (cfg.feature_samples, dim, MAX_FEATURE_SAMPLES, MAX_FEATURE_SAMPLES_WIDE, MAX_CODE_DIM_WIDE))
            # (feature_samples 12 .. 16 run on csrc/corr_wide.hip, which takes any layout with dim <= 128: nothing to warn about - ADVICE round 5)
            if MAX_CODE_DIM_ANY_PATH < dim <= MAX_CODE_DIM and cfg.feature_samples <= MAX_FEATURE_SAMPLES:
                # 72 < dim <= 128 exists on the single-launch forward only (plan_fwd / fused_supported, csrc/c_api.hip,
                # csrc/corr_fused.hip); what it does not take runs on generic_forward like dim > 128 does (fused_kernels_cover decides per
                # call, from the tensors): the same conditions here, with the cfg keys named, as a warning
                from .modules import _pair_set_bound
                why = []
                if cfg.arch != "dino":
                    why.append("cfg.arch is not 'dino' (channels-last feature maps of width 192 / 384 / 768)")
                elif getattr(self.net, "n_feats", 384) not in (192, 384, 768):
                    why.append("cfg.model_type=%s has feature width %d (the single-launch forward takes 192 / 384 / 768)"
                               % (getattr(cfg, "model_type", "?"), self.net.n_feats))
                if cfg.batch_size > _pair_set_bound():
                    why.append("cfg.batch_size = %d exceeds the %d compute units (the tiles of one pair-set run at the same time)"
                               % (cfg.batch_size, _pair_set_bound()))
                if why:
                    import warnings
                    warnings.warn("cfg.dim=%d: code dimensions above %d run on the single-launch forward only, and %s: this configuration "
                                  "runs on ContrastiveCorrelationLoss.generic_forward: same results, several times slower"
                                  % (dim, MAX_CODE_DIM_ANY_PATH, "; ".join(why)))
        # cfg.salience_source: where cfg.use_salience gets its foreground masks - "mask" (batch["mask"], the default) or "attention" (the class
        # token's attention of the backbone, stego_amd.salience: a folder without labels has no other)
        source = getattr(cfg, "salience_source", "mask")
        if source not in ("mask", "attention"):
            raise ValueError("cfg.salience_source = %r, expected 'mask' or 'attention'" % (source,))
        if source == "attention" and getattr(cfg, "cache_backbone_tokens", False):
            raise ValueError("cfg.salience_source = 'attention' needs the backbone's pass over every batch: cached tokens carry no attention "
                             "(cfg.cache_backbone_tokens must be False)")
        if source == "attention" and cfg.use_salience and not hasattr(self.net, "class_attention"):
            raise ValueError("cfg.salience_source = 'attention' needs the DINO featurizer (cfg.arch = 'dino')")
        for p in self.contrastive_corr_loss_fn.parameters():
            p.requires_grad = False
        self.automatic_optimization = False
        self.val_steps = 0
        self.global_step = 0
        self.logged = {}
        self._optims = None
        self._fused = None               # cfg.native_optim: the FusedAdam behind the three optimizers (stego_amd.optim)
        self._reducer = None
        self._augmenter = None
        self._cluster_to_class = None
        # cfg.train_log: the step's statistics stay on the device (stego_amd.step_stats) until the Trainer drains them into `train_log`
        self.train_log = None            # a stego_amd.train_log.TrainLog, set by Trainer.fit
        self._step_stats = None
        self._stats_tags = None
        self._stats_step0 = 0

    def check_cluster_scoring(self):
        """Scoring the cluster probe matches its clusters to the classes one to one: a refitted probe with fewer clusters than classes
        cannot be scored (its pictures can be drawn: the clusters are then coloured by index)."""
        probe_n = getattr(self.cfg, "cluster_probe_n", None)
        if probe_n is not None and int(probe_n) < self.n_classes:
            raise ValueError("cfg.cluster_probe_n = %d is below n_classes = %d: the cluster probe has fewer clusters than the dataset has "
                             "classes and cannot be scored against them (refit it with at least %d clusters)"
                             % (int(probe_n), self.n_classes, self.n_classes))

    @property
    def label_cmap(self):
        """The colormap of the model's dataset as a numpy [n, 3] array, as the reference's attribute (train_segmentation.py:100-103)."""
        from .render import label_cmap
        return label_cmap(self.cfg.dataset_name)

    @property
    def cluster_to_class(self):
        """The class of every cluster of cluster_probe, -1 for none (UnsupervisedMetrics.cluster_to_class()): of the last validation
        or evaluation that computed a Hungarian assignment, else what the checkpoint stored, else None.  demo_segmentation colours
        its cluster pictures with it."""
        for m in (self.test_cluster_metrics, self.cluster_metrics):
            if hasattr(m, "assignments"):
                return m.cluster_to_class()
        return self._cluster_to_class

    # ---- checkpoints in the layout Lightning writes for the reference (train_segmentation.py:106 save_hyperparameters,
    #      :487 ModelCheckpoint) and that eval_segmentation.py:67 / demo_segmentation.py:41 read back with
    #      LitUnsupervisedSegmenter.load_from_checkpoint: a torch-pickled dict with `state_dict` (same keys: the module tree
    #      above is the reference's) and `hyper_parameters = {n_classes, cfg}`
    def checkpoint_dict(self, epoch=0):
        cfg = {k: v for k, v in vars(self.cfg).items()} if not isinstance(self.cfg, dict) else dict(self.cfg)
        ck = {"epoch": int(epoch), "global_step": int(self.global_step), "pytorch-lightning_version": "1.2.10",
              "state_dict": self.state_dict(), "hyper_parameters": {"n_classes": self.n_classes, "cfg": cfg}}
        if self._optims is not None:
            ck["optimizer_states"] = [o.state_dict() for o in self._optims]
        if self.cluster_to_class is not None:
            ck["cluster_to_class"] = [int(c) for c in self.cluster_to_class]
        return ck

    def save_checkpoint(self, path, epoch=0):
        torch.save(self.checkpoint_dict(epoch), path)

    @classmethod
    def load_from_checkpoint(cls, path, map_location="cpu", strict=True, **cfg_overrides):
        """Accepts this build's checkpoints and the reference's Lightning ones (whose `cfg` is an OmegaConf DictConfig
        or a plain dict: anything with .items()).  Keys this build does not have (e.g. torchmetrics buffers) are
        reported, not fatal, with strict=False."""
        ck = torch.load(path, map_location=map_location, weights_only=False)
        hp = ck["hyper_parameters"]
        cfg = hp["cfg"]
        cfg = types.SimpleNamespace(**{k: v for k, v in (cfg.items() if hasattr(cfg, "items") else vars(cfg).items())})
        for k, v in cfg_overrides.items():
            setattr(cfg, k, v)
        model = cls(int(hp["n_classes"]), cfg)
        result = model.load_state_dict(ck["state_dict"], strict=strict)
        model.global_step = int(ck.get("global_step", 0))
        if "optimizer_states" in ck:
            for o, sd in zip(model.optimizers(), ck["optimizer_states"]):
                o.load_state_dict(sd)
        model.load_result = result
        if ck.get("cluster_to_class") is not None:
            model._cluster_to_class = np.asarray(ck["cluster_to_class"], dtype=np.int64)
        return model

    # ---- the slice of the LightningModule protocol the reference uses
    def forward(self, x):
        return self.net(x)[1]

    def log(self, name, value, **_):
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def optimizer_groups(self):
        """The three parameter lists of train_segmentation.py:117-119 with their learning rates: net (+ decoder), linear probe,
        cluster probe."""
        main_params = list(self.net.parameters())
        if self.cfg.rec_weight > 0:
            main_params.extend(self.decoder.parameters())
        return [{"params": main_params, "lr": self.cfg.lr}, {"params": list(self.linear_probe.parameters()), "lr": 5e-3},
                {"params": list(self.cluster_probe.parameters()), "lr": 5e-3}]

    def configure_optimizers(self):
        net_optim, linear_probe_optim, cluster_probe_optim = (torch.optim.Adam(g["params"], lr=g["lr"]) for g in self.optimizer_groups())
        return net_optim, linear_probe_optim, cluster_probe_optim

    def optimizers(self):
        """The three optimizers (net, linear probe, cluster probe).  cfg.native_optim on a HIP device: the three facades of one
        FusedAdam (stego_amd.optim) - built here, or built from the torch optimizers a CPU model has used so far (a checkpoint
        is loaded before the model moves to its device), whose state they take over.  On the CPU the flag changes nothing."""
        if getattr(self.cfg, "native_optim", False) and self._fused is None and self.linear_probe.weight.is_cuda:
            from .optim import FusedAdam
            fused = FusedAdam(self.optimizer_groups(), reducer=self._reducer,
                              zero_grads=getattr(self.cfg, "native_optim_zero", True))
            if self._optims is not None:
                fused.load_state_dict([o.state_dict() for o in self._optims])
            self._fused, self._optims = fused, list(fused.groups)
        if self._optims is None:
            self._optims = list(self.configure_optimizers())
        return self._optims

    def setup_distributed(self):
        """Flat gradient bucket over every trainable parameter + startup broadcast (what DDP does on wrap)."""
        self._reducer = ddp.FlatGradReducer([p for p in self.parameters() if p.requires_grad])
        if self._fused is not None:
            self._fused.use_bucket(self._reducer)
        self._reducer.broadcast_params(0)
        return self._reducer

    def augmenter(self):
        """The maker of img_aug / coord_aug for batches that lack them (cfg.native_aug), seeded from this process's rank."""
        if self._augmenter is None:
            self._augmenter = Augmenter(self.cfg.res, seed=0, rank=int(os.environ.get("RANK", "0")))
        return self._augmenter

    def manual_backward(self, loss):
        """loss.backward() + the DDP gradient exchange (Lightning's manual_backward under accelerator='ddp',
        train_segmentation.py:227): ONE asynchronous averaged all-reduce of the flat bucket; wait_gradients() joins it."""
        loss.backward()
        if self._fused is not None and self._reducer is None:
            self._fused.bucket.reattach()       # the fused step reads the bucket: a replaced .grad is copied into its slot
        if self._reducer is not None:
            self._reducer.reattach()
            # (force_collective: run the collective on a process group of ONE - the single-GPU dress rehearsal of the N > 1 path)
            self._grad_work = self._reducer.allreduce_mean(async_op=True, single_rank_ok=getattr(self, "force_collective", False))

    def wait_gradients(self):
        work, self._grad_work = getattr(self, "_grad_work", None), None
        if work is not None:
            work.wait()                 # stream dependency on RCCL's stream; the host keeps enqueueing

    def training_step(self, batch, batch_idx):
        net_optim, linear_probe_optim, cluster_probe_optim = self.optimizers()
        fused = self._fused
        if fused is not None:
            # cfg.native_optim: the previous fused step left the bucket zeroed; the first step, or native_optim_zero=False: zero it here
            fused.zero_grads = bool(getattr(self.cfg, "native_optim_zero", True))
            if fused.zero_grads and fused.bucket_zeroed:
                fused.zero_uncovered()          # trainable tensors of a shared bucket that no optimizer owns; none without data parallelism
            else:
                fused.zero_grad()
        elif self._reducer is not None:
            self._reducer.zero_grad()
        else:
            net_optim.zero_grad(); linear_probe_optim.zero_grad(); cluster_probe_optim.zero_grad()
        cfg = self.cfg
        with torch.no_grad():
            img, img_pos, label = batch["img"], batch["img_pos"], batch["label"]
        # cfg.cache_backbone_tokens: img / img_pos of a dataset index are the same pixels every epoch -> their frozen-backbone
        # tokens come from the HBM table after the first epoch (featurizers.TokenCache)
        caching = getattr(cfg, "cache_backbone_tokens", False) and getattr(self.net, "token_cache", None) is not None
        # cfg.salience_source "attention": the class token's attention comes out of the two backbone passes the step makes anyway
        attn_salience = bool(cfg.use_salience) and getattr(cfg, "salience_source", "mask") == "attention" and cfg.correspondence_weight > 0
        if attn_salience:
            feats, code, attn = self.net(img, return_attention=True)
            feats_pos, code_pos, attn_pos = self.net(img_pos, return_attention=True)
        else:
            feats, code = self.net(img, cache_index=batch["ind"]) if caching else self.net(img)
            if cfg.correspondence_weight > 0:
                feats_pos, code_pos = self.net(img_pos, cache_index=batch["ind_pos"]) if caching else self.net(img_pos)
        log_args = dict(sync_dist=False, rank_zero_only=True)
        if cfg.use_true_labels:
            signal = one_hot_feats(label + 1, self.n_classes + 1)
            signal_pos = one_hot_feats(batch["label_pos"] + 1, self.n_classes + 1)
        else:
            signal, signal_pos = feats, feats_pos
        loss = 0
        stats_cd = None
        if attn_salience:
            # masks [B, H, W] uint8 at the image's resolution (include/stego_vit.h: stego_attn_salience), batch["mask"] is not read; the
            # native draw takes them as they are, the torch draw gets floats as it does from the loader.  No host synchronisation.
            keep, ps = float(getattr(cfg, "salience_keep", 0.6)), self.net.patch_size
            hw = (img.shape[2] // ps, img.shape[3] // ps)
            salience = attention_salience(attn, hw, ps, keep)[1]
            salience_pos = attention_salience(attn_pos, hw, ps, keep)[1]
            if not getattr(cfg, "native_salience", False):
                salience, salience_pos = salience.float(), salience_pos.float()
        elif cfg.use_salience and getattr(cfg, "salience_source", "mask") == "mask":
            salience = batch["mask"].to(torch.float32).squeeze(1)
            salience_pos = batch["mask_pos"].to(torch.float32).squeeze(1)
        else:
            salience = salience_pos = None

        if cfg.correspondence_weight > 0:
            # train_segmentation.py:163-181.  The three .mean()s of the reference come out of the forward launch itself
            # (ContrastiveCorrelationLoss.total): same values, one dot product instead of a 9 MB reduction + five scalar ops.
            (corr_total, means, pos_intra_cd, pos_inter_cd, neg_inter_cd) = self.contrastive_corr_loss_fn.total(
                signal, signal_pos, salience, salience_pos, code, code_pos,
                (cfg.pos_intra_weight, cfg.pos_inter_weight, cfg.neg_inter_weight))
            pos_intra_loss, pos_inter_loss, neg_inter_loss = means[0], means[1], means[2]
            self.log('loss/pos_intra', pos_intra_loss, **log_args)
            self.log('loss/pos_inter', pos_inter_loss, **log_args)
            self.log('loss/neg_inter', neg_inter_loss, **log_args)
            if getattr(cfg, "train_log", False) and pos_intra_cd.is_cuda:
                # one launch after the last loss term instead of three .mean() here: the means, and on histogram steps the buckets,
                # go into the device ring (include/stego_stats.h); the cd/* entries of `logged` are those of the last drain
                stats_cd = (pos_intra_cd, pos_inter_cd, neg_inter_cd)
            else:
                self.log('cd/pos_intra', pos_intra_cd.mean(), **log_args)
                self.log('cd/pos_inter', pos_inter_cd.mean(), **log_args)
                self.log('cd/neg_inter', neg_inter_cd.mean(), **log_args)
            loss += corr_total * cfg.correspondence_weight

        if cfg.rec_weight > 0:
            if getattr(cfg, "native_rec_loss", False):
                # the same number from one fused call that writes no reconstructed map (include/stego_rec.h)
                rec_loss = native_rec_loss(code, feats, self.decoder)
            else:
                rec_loss = -(norm(self.decoder(code)) * norm(feats)).sum(1).mean()
            self.log('loss/rec', rec_loss, **log_args)
            loss += cfg.rec_weight * rec_loss

        if cfg.aug_alignment_weight > 0 and getattr(cfg, "native_aug", False):
            # the view from the device-side augmentation when the loader did not make it (the synthetic and CPU loaders), and the
            # term with both gradients from one fused call that writes no resized map and no sampled code (include/stego_aug.h)
            if "img_aug" not in batch:
                self.augmenter()(batch)
            _, code_aug = self.net(batch["img_aug"])
            aug_alignment = aug_alignment_loss(code, code_aug, batch["coord_aug"])
            self.log('loss/aug_alignment', aug_alignment, **log_args)
            loss += cfg.aug_alignment_weight * aug_alignment
        elif cfg.aug_alignment_weight > 0:
            _, code_aug = self.net(batch["img_aug"])
            coord = resize(batch["coord_aug"].permute(0, 3, 1, 2), code_aug.shape[2]).permute(0, 2, 3, 1)
            aug_alignment = -torch.einsum("bkhw,bkhw->bhw", norm(sample(code, coord)), norm(code_aug)).mean()
            self.log('loss/aug_alignment', aug_alignment, **log_args)
            loss += cfg.aug_alignment_weight * aug_alignment

        if cfg.crf_weight > 0:
            if getattr(cfg, "native_crf_loss", False):
                # the same number from one fused call that samples only the drawn points (include/stego_crf_loss.h)
                crf = self.crf_loss_fn.mean_loss(img, code, size=56, normalize=True)
            else:
                crf = self.crf_loss_fn(resize(img, 56), norm(resize(code, 56))).mean()
            self.log('loss/crf', crf, **log_args)
            loss += cfg.crf_weight * crf

        # train_segmentation.py:199-224: both probes train on the detached code.  cfg.native_probes: their losses and parameter
        # gradients come from one fused call (include/stego_probe_train.h) instead of the torch chain
        probes = probe_losses if getattr(cfg, "native_probes", False) else torch_probe_losses
        linear_loss, cluster_loss = probes(code, label, self.linear_probe, self.cluster_probe)
        loss += linear_loss
        self.log('loss/linear', linear_loss, **log_args)
        loss += cluster_loss
        self.log('loss/cluster', cluster_loss, **log_args)
        self.log('loss/total', loss, **log_args)
        if stats_cd is not None:
            self._record_stats(stats_cd)

        self.manual_backward(loss)
        self.wait_gradients()
        if fused is not None:
            fused.step()                        # all three groups in one launch (include/stego_optim.h)
        else:
            net_optim.step()
            cluster_probe_optim.step()
            linear_probe_optim.step()

        if cfg.reset_probe_steps is not None and self.global_step == cfg.reset_probe_steps:
            print("RESETTING PROBES")
            self.linear_probe.reset_parameters()
            self.cluster_probe.reset_parameters()
            if fused is not None:
                fused.reset_group(1)
                fused.reset_group(2)
            else:
                self._optims[1] = torch.optim.Adam(list(self.linear_probe.parameters()), lr=5e-3)
                self._optims[2] = torch.optim.Adam(list(self.cluster_probe.parameters()), lr=5e-3)
        self.global_step += 1
        return loss

    def _record_stats(self, cd):
        """cfg.train_log: the three cd tensors and every loss/* scalar of this step into the device ring, in one launch."""
        if self._step_stats is None:
            from .step_stats import StepStats
            freq = max(int(getattr(self.cfg, "scalar_log_freq", 10)), 1)
            self._stats_tags = [k for k, v in self.logged.items() if k.startswith("loss/") and torch.is_tensor(v) and v.is_cuda]
            self._stats_step0 = self.global_step
            self._step_stats = StepStats(len(self._stats_tags), min(max(freq, 4), 64), cd[0].device, n_tensors=3)
        logged = self.logged
        scalars = [logged[k] for k in self._stats_tags]          # (the terms a step logs follow from cfg: the same every step)
        scalars = [v if v.dtype == torch.float32 and v.numel() == 1 else v.float().reshape(1) for v in scalars]
        rank0 = self.train_log is None or self.train_log.writer is not None
        with_hist = rank0 and self.train_log is not None and self.train_log.wants_hist(self.global_step)
        self._step_stats.record([t if t.is_contiguous() else t.contiguous() for t in cd], scalars, with_hist)

    @property
    def stats_drain_every(self):
        """Steps between two drains: cfg.scalar_log_freq, and no more than the ring holds."""
        freq = max(int(getattr(self.cfg, "scalar_log_freq", 10)), 1)
        return min(freq, self._step_stats.ring_slots) if self._step_stats is not None else freq

    def drain_stats(self):
        """One copy of the ring to the host: the cd/* entries of `logged` become the newest means, the records go to `train_log`."""
        if self._step_stats is None:
            return []
        from .train_log import CD_TAGS
        records = self._step_stats.drain()
        for r in records:
            r["step"] += self._stats_step0
        if records:
            for tag, t in zip(CD_TAGS, records[-1]["tensors"]):
                self.logged[tag] = t["mean"]
        if self.train_log is not None:
            self.train_log.consume(records, self._stats_tags)
        return records

    def validation_step(self, batch, batch_idx):
        img, label = batch["img"], batch["label"]
        self.check_cluster_scoring()
        self.net.eval()
        with torch.no_grad():
            _, code = self.net(img)
            n = self.cfg.n_images
            if getattr(self.cfg, "native_metrics", False):
                # both confusion matrices from the low-resolution code in one launch, nothing per pixel and no host sync; the label
                # maps of the n images the caller plots come from the fused head
                from .segment import probe_head
                probe_confusion(self, code, None, label, self.linear_metrics, self.cluster_metrics)
                linear_preds, cluster_preds = probe_head(self, code[:n], None, label.shape[-2:], linear="argmax", cluster="argmax")
                return {'img': img[:n].detach().cpu(), 'linear_preds': linear_preds.cpu(), "cluster_preds": cluster_preds.cpu(),
                        "label": label[:n].detach().cpu()}
            code = F.interpolate(code, label.shape[-2:], mode='bilinear', align_corners=False)
            linear_preds = self.linear_probe(code).argmax(1)
            self.linear_metrics.update(linear_preds, label)
            _, cluster_preds = self.cluster_probe(code, None)
            cluster_preds = cluster_preds.argmax(1)
            self.cluster_metrics.update(cluster_preds, label)
            return {'img': img[:n].detach().cpu(), 'linear_preds': linear_preds[:n].detach().cpu(),
                    "cluster_preds": cluster_preds[:n].detach().cpu(), "label": label[:n].detach().cpu()}

    def validation_epoch_end(self, outputs):
        with torch.no_grad():
            metrics = {**self.linear_metrics.compute(), **self.cluster_metrics.compute()}
            self.linear_metrics.reset()
            self.cluster_metrics.reset()
        self.val_steps += 1
        for k, v in metrics.items():
            self.log(k, v)
        if self.train_log is not None and self.train_log.writer is not None:
            self._log_validation(outputs, metrics)
        return metrics

    def _log_validation(self, outputs, metrics):
        """cfg.train_log, rank 0: what the reference's validation_epoch_end writes (train_segmentation.py:285-330, 361-362) - the 4-row
        sheet of the first validation batch as `plot_labels`, the column-normalised cluster histogram as `conf_matrix` when
        cfg.has_labels and matplotlib is installed, and the metrics once global_step > 2.  (The label-frequency bars are not drawn.)"""
        from .render import comparison_sheet
        from .train_log import confusion_figure
        if outputs:
            o, cmap = outputs[0], self.label_cmap
            sheet = comparison_sheet([{"image": o["img"], "rescale": True}, {"labels": o["label"], "cmap": cmap},
                                      {"labels": o["linear_preds"], "cmap": cmap},
                                      {"labels": o["cluster_preds"], "cmap": cmap, "mapping": self.cluster_metrics.cluster_to_class()}])
            self.train_log.image("plot_labels", sheet, self.global_step)
        if getattr(self.cfg, "has_labels", False) and hasattr(self.cluster_metrics, "histogram"):
            fig = confusion_figure(self.cluster_metrics.histogram.cpu().numpy(), self.label_cmap)
            if fig is not None:
                self.train_log.image("conf_matrix", fig, self.global_step)
        if self.global_step > 2:
            self.train_log.scalars(metrics, self.global_step)


class SyntheticContrastiveDataset(torch.utils.data.Dataset):
    """Offline stand-in for ContrastiveSegDataset (data.py:419-565): same batch keys, seeded random content.
    The 'KNN positive' of image i is a noisy copy of it so that the positive pair is actually related."""

    def __init__(self, n, res, n_classes, seed=0):
        self.n, self.res, self.n_classes, self.seed = n, res, n_classes, seed

    def __len__(self):
        return self.n

    n_cache_items = property(lambda self: 2 * self.n)          # anchors [0, n) + their positives [n, 2n)
    deterministic_items = True                                 # the same index always yields the same pixels
    per_rank = True                                            # my_app seeds it by rank: already a different slice on every rank

    def __getitem__(self, ind):
        g = torch.Generator().manual_seed(self.seed * 100003 + ind)
        img = torch.randn(3, self.res, self.res, generator=g)
        img_pos = img + 0.3 * torch.randn(3, self.res, self.res, generator=g)
        label = torch.randint(0, self.n_classes, (self.res, self.res), generator=g)
        # the positive is a different image: it gets its own index (n + ind), as a real KNN positive has (data.py:547-549),
        # so that anything keyed by index (TokenCache) never confuses it with the anchor
        return dict(ind=ind, img=img, label=label, img_pos=img_pos, ind_pos=self.n + ind, label_pos=label,
                    mask=torch.ones(1, self.res, self.res), mask_pos=torch.ones(1, self.res, self.res))


class Trainer:
    """Minimal stand-in for the Lightning Trainer the reference builds at train_segmentation.py:476-497."""

    def __init__(self, max_steps, device=None, log_every=10, val_loader=None, val_check_interval=None, checkpoint_path=None):
        """val_loader / val_check_interval: every that many steps the model's validation_step runs over val_loader and
        validation_epoch_end reports the metrics (train_segmentation.py:247-330, Trainer(val_check_interval=cfg.val_freq) :489);
        checkpoint_path: rank 0 writes a Lightning-layout checkpoint there after every validation and at the end (the
        ModelCheckpoint callback of :482-486)."""
        self.max_steps, self.log_every = max_steps, log_every
        self.val_loader, self.val_check_interval, self.checkpoint_path = val_loader, val_check_interval, checkpoint_path
        self.val_history = []
        self.rank, self.world, self.local_rank = ddp.init_from_env()
        self.device = device or (torch.device("cuda", self.local_rank) if torch.cuda.is_available() else torch.device("cpu"))

    def fit(self, model, loader):
        model.to(self.device)
        model.train()
        if self.world > 1:
            model.setup_distributed()
        if getattr(model.cfg, "cache_backbone_tokens", False) and hasattr(model.net, "enable_token_cache"):
            # The cache is keyed by dataset index: valid only if an index always yields the same pixels (fixed crops; the
            # reference's random-crop loaders, data.py loader_crop_type "random", re-crop every epoch) and if ind_pos
            # addresses the positive's own pixels.
            ds = loader.dataset
            crop = getattr(model.cfg, "loader_crop_type", "center")
            if not getattr(ds, "deterministic_items", crop != "random"):
                raise ValueError("cfg.cache_backbone_tokens needs a dataset whose items are fixed per index "
                                 "(loader_crop_type=%r re-crops every epoch)" % crop)
            n_items = int(getattr(ds, "n_cache_items", len(ds)))
            model.net.enable_token_cache(n_items, (model.cfg.res, model.cfg.res), self.device)
        logging = bool(getattr(model.cfg, "train_log", False)) and self.device.type == "cuda"
        if logging and model.train_log is None:
            from .train_log import TrainLog
            model.train_log = TrainLog(model.cfg, self.rank)
        loader = self._shard_loader(loader)
        if len(loader) == 0:
            raise ValueError("empty loader (dataset of %d items, batch size %s, drop_last): nothing to train on"
                             % (len(loader.dataset), getattr(loader, "batch_size", "?")))
        step = 0
        epoch = 0
        history = []
        while step < self.max_steps:
            if isinstance(getattr(loader, "sampler", None), torch.utils.data.distributed.DistributedSampler):
                loader.sampler.set_epoch(epoch)      # a new shuffle per epoch, the same on every rank (Lightning does this)
            epoch += 1
            for batch in loader:
                batch = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
                loss = model.training_step(batch, step)
                # the loss stays on the device (a float() here is a host sync every step: the CPU could never run ahead of the GPU);
                # values are read when they are printed and once at the end
                history.append(loss.detach())
                if self.rank == 0 and step % self.log_every == 0:
                    print("step %5d  loss %.5f  " % (step, float(history[-1])) +
                          "  ".join("%s %.5f" % (k, float(v)) for k, v in model.logged.items() if k.startswith("loss/pos") or k.startswith("loss/neg")))
                step += 1
                if step % self.event_check_every == 0 or step >= self.max_steps:
                    self._check_loss_events(step)
                validating = self.val_loader is not None and self.val_check_interval and step % self.val_check_interval == 0
                if logging and (step % model.stats_drain_every == 0 or validating or step >= self.max_steps):
                    model.drain_stats()      # one copy of the ring per log interval: the only time the log waits for the device
                if validating:
                    self._validate(model)
                if step >= self.max_steps:
                    break
        if self.checkpoint_path and self.rank == 0:
            model.save_checkpoint(self.checkpoint_path)
        return [float(v) for v in torch.stack(history).cpu()] if history else []

    event_check_every = 200        # steps between two looks at the loss kernels' event counters (a device -> host copy of a few bytes)
    _events_warned = False

    def _check_loss_events(self, step):
        """The single-launch forward of the correspondence loss has two bounded waits between workgroups; a launch whose workgroups are not
        all on the device at once (another kernel holds compute units: a shared or partitioned device) gives them up and takes its fallback
        paths - same bytes, ~30 us slower per step, and silent.  The library counts those events per workspace; said once here."""
        if self._events_warned or self.device.type != "cuda":
            return
        try:
            from . import capi
            gave_up, repaired = capi.event_counters_total()
        except Exception:       # noqa: BLE001 - a diagnostic must not stop a training run
            return
        if gave_up or repaired:
            import warnings
            self._events_warned = True
            warnings.warn("correspondence loss (rank %d, step %d): %d tiles sampled their anchor themselves and %d old_mean rendezvous timed out "
                          "since the run started - the forward's workgroups are not co-resident (device shared with other kernels, or "
                          "partitioned?).  Results are unaffected; set cfg.shared_device = True (STEGO_FLAG_SHARED_DEVICE) when kernels "
                          "of other streams run beside the loss." % (self.rank, step, gave_up, repaired))

    def _shard_loader(self, loader):
        """Data parallelism needs every rank to see its own slice: a loader without a DistributedSampler over a dataset that is
        not already different per rank (``dataset.per_rank``, the synthetic set is seeded by rank) is rebuilt with one - what
        Lightning's ``replace_sampler_ddp`` does for the reference (train_segmentation.py:461-468)."""
        ds = loader.dataset
        if self.world <= 1 or getattr(ds, "per_rank", False) or \
                isinstance(getattr(loader, "sampler", None), torch.utils.data.distributed.DistributedSampler):
            return loader
        if isinstance(ds, torch.utils.data.IterableDataset):
            raise ValueError("data-parallel training over an IterableDataset: shard it per rank yourself (set dataset.per_rank = True)")
        if loader.batch_size is None:                  # built with batch_sampler=...: batching is not ours to redo
            raise ValueError("data-parallel training needs a loader built with batch_size (not batch_sampler), a DistributedSampler, "
                             "or a dataset with per_rank = True")
        shuffle = isinstance(getattr(loader, "sampler", None), torch.utils.data.RandomSampler)
        # DistributedSampler's default drop_last=False pads the last rank(s) by repeating samples - what Lightning's
        # replace_sampler_ddp gives the reference; whether incomplete BATCHES are dropped stays the loader's own drop_last
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=self.world, rank=self.rank, shuffle=shuffle, seed=0)
        kw = dict(batch_size=loader.batch_size, sampler=sampler, num_workers=loader.num_workers, collate_fn=loader.collate_fn,
                  pin_memory=loader.pin_memory, drop_last=loader.drop_last, timeout=loader.timeout,
                  worker_init_fn=loader.worker_init_fn, generator=loader.generator)
        if loader.num_workers > 0:
            kw.update(prefetch_factor=loader.prefetch_factor, persistent_workers=loader.persistent_workers)
        return torch.utils.data.DataLoader(ds, **kw)

    def _validate(self, model):
        model.eval()
        outs = []
        with torch.no_grad():
            for i, batch in enumerate(self.val_loader):
                batch = {k: (v.to(self.device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
                outs.append(model.validation_step(batch, i))
        metrics = model.validation_epoch_end(outs)
        self.val_history.append(metrics)
        model.train()
        if self.checkpoint_path and self.rank == 0:
            model.save_checkpoint(self.checkpoint_path)
        return metrics


def checkpoint_path(cfg):
    """Where my_app's Trainer writes the checkpoint of a run on real data (the reference's ModelCheckpoint dirpath,
    {output_root}/checkpoints/{log_dir}/..., train_segmentation.py:393-396,482-486)."""
    return join(cfg.output_root, "checkpoints", str(cfg.log_dir), "{}_{}.ckpt".format(cfg.dataset_name, cfg.experiment_name))


def _real_loaders(cfg, trainer):
    """train_segmentation.py:421-457 on the cropped tree: the training loader (the device store when cfg.device_dataset and the split
    fits cfg.device_dataset_max_gb, else ContrastiveSegDataset on cfg.num_workers CPU workers) and the val loader (the cropped val
    split at 320, centre crops; the reference's raw-COCO val reader is not part of this build)."""
    import numpy as np
    from .data import ContrastiveSegDataset, crop_dir, image_transform, label_transform
    from .device_data import DeviceContrastiveLoader, DeviceImageStore, StoreTooLarge
    from .precompute_knns import nns_filename
    root = cfg.pytorch_data_dir
    crop = getattr(cfg, "loader_crop_type", "center")
    nns_path = join(root, "nns", nns_filename(cfg.model_type, cfg.dataset_name, "train", cfg.crop_type, cfg.res))
    loader = None
    if getattr(cfg, "device_dataset", True):
        max_bytes = float(getattr(cfg, "device_dataset_max_gb", 200)) * 2 ** 30
        try:
            store = DeviceImageStore(root, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio, "train", device=trainer.device,
                                     max_bytes=max_bytes)
        except StoreTooLarge as e:
            print("training data: CPU loader (ContrastiveSegDataset, %d workers): %s (cfg.device_dataset_max_gb = %s)"
                  % (cfg.num_workers, e, cfg.device_dataset_max_gb))
        else:
            if not os.path.exists(nns_path):
                raise ValueError("could not find nn file {} please run precompute_knns".format(nns_path))
            loader = DeviceContrastiveLoader(store, np.load(nns_path)["nns"], cfg.batch_size, cfg.num_neighbors, cfg.res, crop=crop,
                                             seed=0, rank=trainer.rank, world=trainer.world, drop_last=True,
                                             aug=cfg.aug_alignment_weight > 0 and getattr(cfg, "native_aug", False))
            print("training data: device store (%d crops, %.2f GB on the device)" % (len(store), store.nbytes / 1e9))
    else:
        print("training data: CPU loader (ContrastiveSegDataset, %d workers): cfg.device_dataset is off" % cfg.num_workers)
    if loader is None:
        ds = ContrastiveSegDataset(root, cfg.dataset_name, cfg.crop_type, "train", image_transform(cfg.res, crop),
                                   label_transform(cfg.res, crop), cfg, num_neighbors=cfg.num_neighbors, mask=True, pos_images=True,
                                   pos_labels=True)
        loader = torch.utils.data.DataLoader(ds, cfg.batch_size, shuffle=True, num_workers=cfg.num_workers, pin_memory=True,
                                             drop_last=True)
    val_loader = None
    if os.path.exists(join(crop_dir(root, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio), "img", "val")):
        if getattr(cfg, "device_dataset", True):
            try:
                vstore = DeviceImageStore(root, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio, "val", device=trainer.device,
                                          max_bytes=float(getattr(cfg, "device_dataset_max_gb", 200)) * 2 ** 30)
                val_loader = DeviceContrastiveLoader(vstore, None, cfg.batch_size, res=320, drop_last=False)
            except StoreTooLarge as e:
                print("val data: CPU loader: %s" % e)
        if val_loader is None:
            vds = ContrastiveSegDataset(root, cfg.dataset_name, cfg.crop_type, "val", image_transform(320), label_transform(320), cfg,
                                        mask=True)
            val_loader = torch.utils.data.DataLoader(vds, cfg.batch_size, shuffle=False, num_workers=cfg.num_workers, pin_memory=True)
    else:
        print("no cropped val split: training without validation")
    return loader, val_loader


def _directory_loaders(cfg, trainer):
    """_real_loaders for dataset_name "directory" (the image folder {pytorch_data_dir}/{dir_dataset_name}, data.DirectoryDataset).
    The training loader is, in this order: the device store at full size when it fits cfg.device_dataset_max_gb; else the device store
    reduced to store_res = cfg.res (bitwise the same batches); else ContrastiveSegDataset on cfg.num_workers CPU workers.  Validation
    (centre crops at 320) runs only when the folder has both imgs/val and labels/val."""
    import numpy as np
    from .data import ContrastiveSegDataset, image_transform, label_transform
    from .device_data import DeviceContrastiveLoader, DeviceImageStore, StoreTooLarge
    from .precompute_knns import nns_path
    root, name = cfg.pytorch_data_dir, cfg.dir_dataset_name
    crop = getattr(cfg, "loader_crop_type", "center")
    max_gb = getattr(cfg, "device_dataset_max_gb", 200)
    max_bytes = float(max_gb) * 2 ** 30
    table = nns_path(cfg, "train", cfg.res)
    if not os.path.exists(join(root, name, "labels")):
        print("training data: %s has no labels folder: every label is -1, so loss/linear and loss/total are NaN (no valid pixel: NaN "
              "loss, zero gradients, as F.cross_entropy gives the reference); every gradient stays finite and the cluster probe and "
              "the correspondence losses train as usual" % join(root, name))
    loader = None
    if getattr(cfg, "device_dataset", True):
        store = None
        try:
            store = DeviceImageStore.from_directory(root, name, "train", device=trainer.device, max_bytes=max_bytes)
            print("training data: device store of the folder at full size (%d images, %.2f GB on the device)" % (len(store), store.nbytes / 1e9))
        except StoreTooLarge as e:
            try:
                store = DeviceImageStore.from_directory(root, name, "train", device=trainer.device, max_bytes=max_bytes, store_res=cfg.res)
                print("training data: device store reduced to store_res = %d (%d images, %.2f GB on the device): %s "
                      "(cfg.device_dataset_max_gb = %s)" % (cfg.res, len(store), store.nbytes / 1e9, e, max_gb))
            except StoreTooLarge as e2:
                print("training data: CPU loader (ContrastiveSegDataset, %d workers): %s (cfg.device_dataset_max_gb = %s)"
                      % (cfg.num_workers, e2, max_gb))
        if store is not None:
            if not os.path.exists(table):
                raise ValueError("could not find nn file {} please run precompute_knns".format(table))
            loader = DeviceContrastiveLoader(store, np.load(table)["nns"], cfg.batch_size, cfg.num_neighbors, cfg.res, crop=crop,
                                             seed=0, rank=trainer.rank, world=trainer.world, drop_last=True,
                                             aug=cfg.aug_alignment_weight > 0 and getattr(cfg, "native_aug", False))
    else:
        print("training data: CPU loader (ContrastiveSegDataset, %d workers): cfg.device_dataset is off" % cfg.num_workers)
    if loader is None:
        ds = ContrastiveSegDataset(root, "directory", None, "train", image_transform(cfg.res, crop), label_transform(cfg.res, crop), cfg,
                                   num_neighbors=cfg.num_neighbors, mask=True, pos_images=True, pos_labels=True)
        loader = torch.utils.data.DataLoader(ds, cfg.batch_size, shuffle=True, num_workers=cfg.num_workers, pin_memory=True,
                                             drop_last=True)
    val_loader = None
    if os.path.exists(join(root, name, "imgs", "val")) and os.path.exists(join(root, name, "labels", "val")):
        if getattr(cfg, "device_dataset", True):
            try:
                vstore = DeviceImageStore.from_directory(root, name, "val", device=trainer.device, max_bytes=max_bytes, store_res=320)
                val_loader = DeviceContrastiveLoader(vstore, None, cfg.batch_size, res=320, drop_last=False)
            except StoreTooLarge as e:
                print("val data: CPU loader: %s" % e)
        if val_loader is None:
            vds = ContrastiveSegDataset(root, "directory", None, "val", image_transform(320), label_transform(320), cfg, mask=True)
            val_loader = torch.utils.data.DataLoader(vds, cfg.batch_size, shuffle=False, num_workers=cfg.num_workers, pin_memory=True)
    else:
        print("no labelled val split in the folder: training without validation")
    return loader, val_loader


def my_app(cfg):
    """Trains on the cropped tree {pytorch_data_dir}/cropped/{dataset}_{crop_type}_crop_{ratio} when its train split exists (KNN
    positives from precompute_knns' table), on the image folder {pytorch_data_dir}/{dir_dataset_name} for dataset_name "directory"
    (n_classes = cfg.dir_dataset_n_classes), on synthetic data otherwise.  Returns the per-step losses."""
    from .data import crop_dir
    torch.manual_seed(0)            # seed_everything(0), train_segmentation.py:403
    root = getattr(cfg, "pytorch_data_dir", None)
    if cfg.dataset_name == "directory":
        n_classes = int(cfg.dir_dataset_n_classes)
        if not root or not os.path.exists(join(root, cfg.dir_dataset_name, "imgs", "train")):
            raise ValueError("dataset_name directory: no folder %s" % join(str(root), str(cfg.dir_dataset_name), "imgs", "train"))
        if getattr(cfg, "loader_crop_type", "center") not in ("center", "random"):
            raise ValueError("loader_crop_type %r is not supported (center or random)" % cfg.loader_crop_type)
        real = _directory_loaders
    else:
        n_classes = get_class_labels(cfg.dataset_name)
        real = _real_loaders
    if cfg.dataset_name == "directory" or \
            (root and os.path.exists(join(crop_dir(root, cfg.dataset_name, cfg.crop_type, cfg.crop_ratio), "img", "train"))):
        refusal = needs_torchvision(cfg)
        if refusal:
            raise ValueError(refusal)
        import random
        import numpy as np
        random.seed(0)
        np.random.seed(0)
        ckpt = checkpoint_path(cfg)
        os.makedirs(dirname(ckpt), exist_ok=True)
        trainer = Trainer(cfg.max_steps, log_every=cfg.scalar_log_freq, val_check_interval=cfg.val_freq, checkpoint_path=ckpt)
        loader, trainer.val_loader = real(cfg, trainer)
        model = LitUnsupervisedSegmenter(n_classes, cfg)
        return trainer.fit(model, loader)
    trainer = Trainer(cfg.max_steps)
    ds = SyntheticContrastiveDataset(max(cfg.batch_size * 8, 64), cfg.res, n_classes, seed=trainer.rank)
    loader = torch.utils.data.DataLoader(ds, cfg.batch_size, shuffle=True, num_workers=0, drop_last=True)
    model = LitUnsupervisedSegmenter(n_classes, cfg)
    return trainer.fit(model, loader)


if __name__ == "__main__":
    prep_args()
    my_app(load_config(overrides=sys.argv[1:]))

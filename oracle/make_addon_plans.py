"""Record tests/golden/addon_plans.json: everything the host-only `*_workspace_bytes` and `*_plan` exports of the add-on units return for
a table of descriptors (tests/test_addon_plans_host.py asserts exact equality).  The fixture is data: function name, the descriptor's
arguments, the returned numbers.  Record it from the library of the commit whose numbers are to be pinned, no device is needed:

    python -m oracle.make_addon_plans [out.json]

The table sits at the edges where a workspace layout or a tile plan can go wrong, not at workload sizes: K around the 32-channel tiles,
point / token / cell counts at 1 and one off the stage sizes (128 rows, 32 tokens, 16 cells), C around 32 and at the limit, B at 1, 2 and
65535, 0 / 1 / 8 / 9 / 64 labels per probe, heatmap widths that are and are not a multiple of 4, and a few descriptors the units refuse.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "addon_plans.json")

KS = (1, 31, 32, 33, 64, 65, 128)
CS = (1, 31, 32, 33, 1024)
BS = (1, 2, 65535)
LABELS = [(a, b) for a in (0, 1, 8, 9, 64) for b in (0, 1, 8, 9, 64) if a or b]
CRF = (0.5, 0.15, 0.25, 10.0, 3.0, 0.0)      # alpha, beta, gamma, w1, w2, shift: no size depends on them

# function -> (descriptor constructor, workspace-size function or None, plan function), all names of stego_amd.capi
FUNCS = {
    "crf_loss": ("crf_loss_desc", "crf_loss_workspace_bytes", "crf_loss_plan"),
    "augment": ("aug_desc", "augment_workspace_bytes", "augment_plan"),
    "aug_align": ("aug_align_desc", "aug_align_workspace_bytes", "aug_align_plan"),
    "rec_loss": ("rec_desc", "rec_loss_workspace_bytes", "rec_loss_plan"),
    "probe_train": ("probe_train_desc", "probe_train_workspace_bytes", "probe_train_plan"),
    "heat": ("heat_desc", "heat_workspace_bytes", "heat_plan"),
    "probe_head": ("probe_desc", None, "probe_head_plan"),
    "stitch_probe": ("stitch_desc", None, "stitch_probe_plan"),
    "probe_confusion": ("probe_confusion_desc", None, "probe_confusion_plan"),
    "pr": ("pr_desc", None, "pr_plan"),
}


def table():
    rows = []

    def add(fn, *args):
        rows.append((fn, list(args)))

    # crf_loss(B, K, G, h, w, hg, wg, H, W, N, alpha, beta, gamma, w1, w2, shift): stages of CB = 128 points, 16 cells per finish unit
    for K in KS:
        for N in (1, 63, 64, 65, 127, 128, 129, 4096):
            add("crf_loss", 1, K, 3, 4, 4, 9, 9, 32, 32, N, *CRF)
    for B in BS:
        for h, w in ((1, 1), (3, 5), (4, 4), (1, 17), (28, 28)):
            add("crf_loss", B, 33, 8, h, w, 7, 5, 224, 224, 129, *CRF)
    add("crf_loss", 1, 0, 3, 4, 4, 9, 9, 32, 32, 16, *CRF)
    add("crf_loss", 1, 129, 3, 4, 4, 9, 9, 32, 32, 16, *CRF)
    add("crf_loss", 1, 16, 3, 4, 4, 9, 9, 32, 32, 4097, *CRF)
    # augment(B, H, W, R): 8 rows per mean workgroup, 16 x 64 tiles
    for B in BS:
        for R in (3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 224, 2048):
            add("augment", B, 40, 50, R)
    add("augment", 1, 40, 50, 2)
    # aug_align(B, K, h, w, S, Rh, Rw): four pixels per workgroup, 16 cells per finish unit
    for K in KS:
        for S in (1, 2, 3, 8, 9, 256):
            add("aug_align", 2, K, 4, 4, S, 32, 24)
    for B in BS:
        for h, w in ((1, 1), (3, 5), (4, 4), (1, 17)):
            add("aug_align", B, 65, h, w, 3, 7, 224)
    add("aug_align", 1, 129, 4, 4, 3, 7, 7)
    # rec_loss(B, K, C, h, w): tiles of 32 tokens, at most 2048 tile workgroups and 64 token ranges
    for K in KS:
        for C in CS:
            add("rec_loss", 1, K, C, 5, 7)
    for B, h, w in ((1, 1, 1), (1, 1, 31), (1, 4, 8), (1, 3, 11), (2, 28, 28), (1, 1, 2016), (1, 32, 64), (1, 3, 683), (65535, 1, 1),
                    (65535, 16, 16), (1, 2048, 2048), (2, 2048, 2048)):
        add("rec_loss", B, 33, 33, h, w)
    add("rec_loss", 1, 33, 1025, 5, 7)
    add("rec_loss", 65535, 33, 33, 16, 17)
    # probe_train(B, K, h, w, H, W, n_lin, n_clu)
    for K in KS:
        add("probe_train", 2, K, 7, 5, 33, 65, 9, 8)
    for n_lin, n_clu in LABELS:
        add("probe_train", 2, 33, 7, 5, 33, 65, n_lin, n_clu)
    for B in BS:
        for h, w, H, W in ((1, 1, 1, 1), (28, 28, 224, 224), (7, 5, 33, 65), (40, 40, 320, 320), (65535, 1, 2048, 3)):
            add("probe_train", B, 70, h, w, H, W, 27, 27)
    add("probe_train", 1, 70, 7, 5, 33, 65, 0, 0)
    add("probe_train", 1, 70, 7, 5, 33, 65, 65, 0)
    # heat(B, C, hs, ws, h, w, N, H, W): chunks of 128 cells, tiles of 128 queries, 16-byte stores when W % 4 == 0
    for C in (1, 31, 32, 33, 768):
        add("heat", 2, C, 9, 7, 8, 16, 5, 32, 32)
    for h, w in ((1, 1), (1, 127), (8, 16), (3, 43), (128, 128)):
        for N in (1, 127, 128, 129, 4096):
            add("heat", 1, 33, 9, 7, h, w, N, 17, 20)
    for B in BS:
        for H, W in ((1, 1), (5, 7), (8, 8), (224, 224), (17, 2048), (2048, 3), (33, 6)):
            add("heat", B, 33, 9, 7, 28, 28, 3, H, W)
    add("heat", 1, 769, 9, 7, 8, 16, 5, 32, 32)
    add("heat", 1, 33, 9, 7, 128, 129, 5, 32, 32)
    # probe_head(B, K, h, w, H, W, n_lin, n_clu, lin_kind, clu_kind, alpha): kinds 0 skip, 1 log_probs, 3 argmax
    for K in KS:
        add("probe_head", 2, K, 7, 5, 33, 65, 9, 8, 1, 3, 3.0)
    for n_lin, n_clu in LABELS:
        add("probe_head", 2, 33, 7, 5, 33, 65, n_lin, n_clu, 1 if n_lin else 0, 3 if n_clu else 0, 3.0)
    for B in BS:
        for h, w, H, W in ((1, 1, 1, 1), (28, 28, 224, 224), (40, 40, 320, 320), (65535, 1, 2048, 3), (300, 300, 64, 64)):
            add("probe_head", B, 128, h, w, H, W, 64, 64, 2, 2, 3.0)
    add("probe_head", 1, 33, 7, 5, 33, 65, 9, 8, 0, 0, 3.0)
    add("probe_head", 1, 33, 7, 5, 33, 65, 65, 8, 1, 1, 3.0)
    # stitch_probe(H, W, win, stride, T, K, hc, wc, n_lin, n_clu, lin_kind, clu_kind, alpha)
    for K in KS:
        add("stitch_probe", 500, 333, 224, 112, 12, K, 28, 28, 9, 8, 1, 3, 3.0)
    for n_lin, n_clu in LABELS:
        add("stitch_probe", 500, 333, 224, 112, 12, 33, 28, 28, n_lin, n_clu, 1 if n_lin else 0, 3 if n_clu else 0, 3.0)
    for H, W, win, stride, hc, wc in ((1, 1, 1, 1, 1, 1), (224, 224, 224, 224, 28, 28), (225, 224, 224, 112, 28, 28), (32768, 32768, 2048, 1024, 256, 256),
                                      (100, 90, 33, 17, 300, 300), (64, 65, 64, 63, 7, 5)):
        add("stitch_probe", H, W, win, stride, 1, 128, hc, wc, 64, 64, 2, 2, 3.0)
    add("stitch_probe", 500, 333, 224, 111, 12, 33, 28, 28, 9, 8, 1, 3, 3.0)
    # probe_confusion(B, K, h, w, H, W, n_lin, n_clu, lin_on, clu_on, alpha, n_classes)
    for K in KS:
        add("probe_confusion", 2, K, 7, 5, 33, 65, 9, 8, 1, 1, 3.0, 27)
    for n_lin, n_clu in LABELS:
        for n_classes in (1, 64):
            add("probe_confusion", 2, 33, 7, 5, 33, 65, n_lin, n_clu, 1 if n_lin else 0, 1 if n_clu else 0, 3.0, n_classes)
    for B in BS:
        for h, w, H, W in ((1, 1, 1, 1), (28, 28, 224, 224), (65535, 1, 2048, 3), (300, 300, 64, 64)):
            add("probe_confusion", B, 128, h, w, H, W, 64, 64, 1, 1, 3.0, 64)
    add("probe_confusion", 1, 33, 7, 5, 33, 65, 9, 8, 0, 0, 3.0, 27)
    # pr(B, C, h, w, HL, WL, N1, N2, n_bins, n_classes, flags)
    for C in (1, 31, 32, 33, 768):
        for n_bins in (64, 65, 8192):
            add("pr", 2, C, 28, 28, 224, 224, 121, 121, n_bins, 27, 0)
    for N1 in (1, 127, 128, 129, 4096):
        for N2 in (1, 129, 4096):
            add("pr", 1, 33, 7, 5, 33, 65, N1, N2, 100, 255, 3)
    for B in BS:
        add("pr", B, 70, 1, 1, 1, 1, 16, 16, 64, 1, 0)
    add("pr", 1, 769, 28, 28, 224, 224, 121, 121, 100, 27, 0)
    add("pr", 1, 33, 28, 28, 224, 224, 121, 121, 63, 27, 0)
    return rows


def evaluate(capi, fn, args):
    """What the two exports return for one row, in JSON's types."""
    ctor, ws_fn, plan_fn = FUNCS[fn]
    desc = getattr(capi, ctor)(*args)
    got = {"ws": getattr(capi, ws_fn)(desc) if ws_fn else None, "plan": getattr(capi, plan_fn)(desc)}
    return json.loads(json.dumps(got))


def main(out=OUT):
    sys.path.insert(0, ROOT)
    from stego_amd import capi
    rows = [dict(fn=fn, args=args, **evaluate(capi, fn, args)) for fn, args in table()]
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows -> %s" % (len(rows), out))


if __name__ == "__main__":
    main(*sys.argv[1:2])

"""Host-side contract of the fused reconstruction loss (include/stego_rec.h): the exported symbols and the ctypes binding against the
header, every limit of the descriptor and its error code, the workspace and the plan, tests/rec_oracle.py against torch's float64
autograd and the golden file made from the reference's own lines, the conditioning of the GPU test's case table, and the fallback rule
of stego_amd.rec_loss.rec_loss.  No GPU: every call here fails one of the host's checks and returns before anything is enqueued."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import rec_oracle
from stego_amd import capi
from stego_amd.rec_loss import rec_loss, torch_rec_loss
from test_rec_loss_gpu import CASES, WELL_CONDITIONED, allowance_used, chain_grad, make_inputs, reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "stego_rec.h")).read()
A, BIG = 4096, 1 << 40                       # a plausible aligned address: nothing dereferences it before the checks return
NAMES = ("code", "feats", "weight", "bias", "loss", "d_code", "d_weight", "d_bias", "workspace")
MAPS = ("code", "feats", "d_code")


def _desc(**kw):
    d = dict(B=2, K=70, C=384, h=28, w=28)
    d.update(kw)
    return capi.rec_desc(d["B"], d["K"], d["C"], d["h"], d["w"])


def _rec_rc(desc, workspace_bytes=BIG, **kw):
    a = dict.fromkeys(NAMES, A)
    for n in MAPS:
        a[n] = capi.StegoMap(A, 70 * 784, 784, 28, 1)
    a.update(kw)
    return capi.rec_loss_raw(desc, *[a[n] for n in NAMES], workspace_bytes)


def test_symbols_signatures_and_the_descriptor_match_the_header():
    lib = capi.load()
    for name in ("stego_rec_loss_workspace_bytes", "stego_rec_loss_plan", "stego_rec_loss"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and re.search(r"\b%s\(" % name, HEADER), name
    body = re.search(r"typedef struct StegoRecDesc \{(.*?)\} StegoRecDesc;", HEADER, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == [n for n, _ in capi.StegoRecDesc._fields_] == ["B", "K", "C", "h", "w"]
    assert all(t is ctypes.c_int32 for _, t in capi.StegoRecDesc._fields_) and ctypes.sizeof(capi.StegoRecDesc) == 20
    decl = re.search(r"int stego_rec_loss\((.*?)\);", HEADER, re.S).group(1)
    assert len(decl.split(",")) == len(capi.SIGNATURES["stego_rec_loss"][1]) == 12
    assert capi.SIGNATURES["stego_rec_loss"][1][1:3] == [capi._M, capi._M] and capi.SIGNATURES["stego_rec_loss"][1][6] is capi._M
    assert lib.stego_abi_version() == 7 == capi.ABI_VERSION


def test_error_codes_limits_and_error_strings_match_the_header():
    codes = dict(re.findall(r"(STEGO_ERR_REC_\w+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in codes.items()} == {"STEGO_ERR_REC_DIM": capi.REC_ERR_DIM, "STEGO_ERR_REC_SIZE": capi.REC_ERR_SIZE}
    assert (capi.REC_ERR_DIM, capi.REC_ERR_SIZE) == (140, 141)
    defines = {k: eval(v) for k, v in re.findall(r"#define (STEGO_REC_\w+) (\(1 << \d+\)|\d+)", HEADER)}
    assert defines == {"STEGO_REC_MAX_K": capi.REC_MAX_K, "STEGO_REC_MAX_C": capi.REC_MAX_C, "STEGO_REC_MAX_B": capi.REC_MAX_B,
                       "STEGO_REC_MAX_SIDE": capi.REC_MAX_SIDE, "STEGO_REC_MAX_TOKENS": capi.REC_MAX_TOKENS, "STEGO_REC_TILE": capi.REC_TILE,
                       "STEGO_REC_MAX_WORKGROUPS": capi.REC_MAX_WORKGROUPS, "STEGO_REC_LAUNCHES": capi.REC_LAUNCHES}
    assert (capi.REC_MAX_K, capi.REC_MAX_C, capi.REC_MAX_B, capi.REC_MAX_SIDE, capi.REC_MAX_TOKENS) == (128, 1024, 65535, 2048, 1 << 24)
    for code in (capi.REC_ERR_DIM, capi.REC_ERR_SIZE):
        assert capi.load().stego_error_string(code).decode().startswith("rec loss:")


@pytest.mark.parametrize("kw,rc", [
    (dict(K=0), capi.REC_ERR_DIM), (dict(K=129), capi.REC_ERR_DIM), (dict(C=0), capi.REC_ERR_DIM), (dict(C=1025), capi.REC_ERR_DIM),
    (dict(B=0), capi.REC_ERR_SIZE), (dict(B=65536), capi.REC_ERR_SIZE), (dict(h=0), capi.REC_ERR_SIZE), (dict(h=2049), capi.REC_ERR_SIZE),
    (dict(w=0), capi.REC_ERR_SIZE), (dict(w=2049), capi.REC_ERR_SIZE),
    (dict(B=5, h=2048, w=2048), capi.REC_ERR_SIZE), (dict(B=4, h=2048, w=2048, K=1, C=1), 0), (dict(B=65535, h=16, w=16), 0),
    (dict(B=65535, h=16, w=17), capi.REC_ERR_SIZE), (dict(K=128, C=1024), 0), (dict(K=1, C=1, B=1, h=1, w=1), 0),
])
def test_descriptor_checks(kw, rc):
    if rc != 0:                                  # (a valid call would be enqueued: the addresses here are not memory)
        assert _rec_rc(_desc(**kw)) == rc
    assert (capi.rec_loss_workspace_bytes(_desc(**kw)) == 0) == (rc != 0)
    plan = capi.rec_loss_plan(_desc(**kw))
    assert plan[0] == rc and (plan[1] == [(0, 0)] * 2) == (rc != 0)


@pytest.mark.parametrize("which", [n for n in NAMES if not n.startswith("d_")])
def test_null_pointers(which):
    assert _rec_rc(_desc(), **{which: None}) == 1
    if which in MAPS:
        assert _rec_rc(_desc(), **{which: capi.StegoMap(0, 1, 1, 1, 1)}) == 1


def test_null_descriptor_and_optional_gradients():
    m = capi.StegoMap(A, 1, 1, 1, 1)
    assert capi.rec_loss_raw(None, m, m, A, A, A, None, None, None, A, BIG) == 1
    assert capi.rec_loss_workspace_bytes(_desc()) > 0 and capi.load().stego_rec_loss_workspace_bytes(None) == 0
    assert _rec_rc(_desc(), d_code=capi.StegoMap(0, 1, 1, 1, 1)) == 1               # a d_code map without data
    assert _rec_rc(_desc(), d_code=None, d_weight=None, d_bias=None, workspace_bytes=0) == 4     # NULL gradients pass the pointer checks


def test_short_workspace_and_alignment():
    need = capi.rec_loss_workspace_bytes(_desc())
    assert _rec_rc(_desc(), workspace_bytes=need - 1) == 4                            # STEGO_ERR_WORKSPACE
    for which in NAMES:
        bad = capi.StegoMap(A + 2, 70 * 784, 784, 28, 1) if which in MAPS else A + 2
        assert _rec_rc(_desc(), **{which: bad}) == 5, which                           # STEGO_ERR_ALIGN
    assert _rec_rc(_desc(), workspace=A + 8) == 5                                     # the workspace: 16 bytes


def test_workspace_and_plan():
    ws = [capi.rec_loss_workspace_bytes(_desc(B=b)) for b in (1, 2, 3, 8, 32, 33, 64, 1000)]
    assert ws == sorted(ws) and ws[0] > 0
    ws = [capi.rec_loss_workspace_bytes(_desc(C=c)) for c in (1, 31, 32, 33, 65, 384, 385, 768, 1024)]
    assert ws == sorted(ws)
    train = _desc(B=32)
    feats_bytes = 32 * 384 * 28 * 28 * 4
    share = capi.rec_loss_workspace_bytes(train) / feats_bytes
    print("workspace at B = 32, K = 70, C = 384, 28 x 28: %d bytes = %.3f of feats" % (capi.rec_loss_workspace_bytes(train), share))
    assert capi.rec_loss_workspace_bytes(train) == 7186608 and share < 0.25
    for d in (train, _desc(K=128, C=1024), _desc(K=1, C=1, B=1, h=1, w=1), _desc(B=3, K=33, C=96, h=7, w=5)):
        rc, launches = capi.rec_loss_plan(d)
        print("plan (B %d, K %d, C %d, %d x %d): %s" % (d.B, d.K, d.C, d.h, d.w, launches))
        assert rc == 0 and len(launches) == capi.REC_LAUNCHES == 2
        tiles = -(-d.B * d.h * d.w // capi.REC_TILE)
        ranges, chunks = min(tiles, capi.REC_MAX_WORKGROUPS), -(-d.C // 32)
        assert launches[0][1] == min(tiles, 2048) and launches[1][1] == ranges * chunks + 1
        assert all(0 < lds <= 160 * 1024 for lds, _ in launches)


def _oracle_close(got, want, what, tol=1e-12):
    err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / max(float(np.max(np.abs(want))), 1e-300)
    print("%s: max|a - e| / max|e| = %.3e" % (what, err))
    assert err <= tol, (what, err)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_numpy_oracle_agrees_with_float64_autograd(case):
    inputs = make_inputs(case)
    got = rec_oracle.rec_loss(*[t.double().numpy() for t in inputs])
    ref = reference(case)
    code, feats, weight, bias = (t.double() for t in inputs)
    dec = nn.Conv2d(weight.shape[1], weight.shape[0], 1).double()
    with torch.no_grad():
        dec.weight.copy_(weight.reshape(dec.weight.shape))
        dec.bias.copy_(bias)
    _oracle_close(torch_rec_loss(code, feats, dec).item(), ref[0], "case %d torch_rec_loss" % case)
    for a, e, name in zip(got, ref, ("loss", "d_code", "d_weight", "d_bias")):
        _oracle_close(a, e, "case %d %s" % (case, name))


def test_zero_tokens_in_the_oracle():
    """The clamp rule: below eps the projection vanishes; a zero feature contributes nothing."""
    code, feats, weight, bias = (t.clone() for t in make_inputs(4))
    bias.zero_()
    feats[0, :, 1, 2] = 0.0
    code[1, :, 2, 1] = 0.0
    ref = chain_grad((code, feats, weight, bias), torch.float64)
    got = rec_oracle.rec_loss(*[t.double().numpy() for t in (code, feats, weight, bias)])
    for a, e, name in zip(got, ref, ("loss", "d_code", "d_weight", "d_bias")):
        _oracle_close(a, e, "zero tokens %s" % name)
    assert np.isfinite(got[1]).all() and (got[1][0, :, 1, 2] == 0).all()


def test_golden_file_from_the_reference_lines():
    z = np.load(os.path.join(ROOT, "tests", "golden", "rec_loss_small.npz"))
    assert z["code"].shape == (2, 5, 4, 3) and z["feats"].shape == (2, 12, 4, 3) and z["code"].dtype == np.float64
    got = rec_oracle.rec_loss(z["code"], z["feats"], z["weight"], z["bias"])[0]
    dec = nn.Conv2d(5, 12, 1).double()
    with torch.no_grad():
        dec.weight.copy_(torch.from_numpy(z["weight"]).reshape(12, 5, 1, 1))
        dec.bias.copy_(torch.from_numpy(z["bias"]))
        chain = torch_rec_loss(torch.from_numpy(z["code"]), torch.from_numpy(z["feats"]), dec).item()
    print("golden loss %.17g oracle %.17g torch_rec_loss %.17g" % (float(z["loss"]), got, chain))
    assert abs(got - float(z["loss"])) <= 1e-14 and abs(chain - float(z["loss"])) <= 1e-14


@pytest.mark.parametrize("case", WELL_CONDITIONED)
def test_torch_fp32_uses_a_quarter_of_the_allowance_at_most(case):
    """Guards the case table, not the kernel: the cases held to assert_close are well conditioned."""
    got, ref = chain_grad(make_inputs(case), torch.float32), reference(case)
    used = [allowance_used(a, e) for a, e in zip(got, ref)]
    print("case %d: torch fp32 uses loss %.4f d_code %.4f d_weight %.4f d_bias %.4f of the allowance" % ((case,) + tuple(used)))
    assert max(used) <= 0.25


def test_rec_loss_on_cpu_tensors_is_the_torch_chain():
    code, feats, weight, bias = make_inputs(2)
    dec = nn.Conv2d(33, 96, 1)
    with torch.no_grad():
        dec.weight.copy_(weight.reshape(dec.weight.shape))
        dec.bias.copy_(bias)
    for f in (feats, feats.clone().requires_grad_(True)):
        x = code.clone().requires_grad_(True)
        a = rec_loss(x, f, dec)
        ga = torch.autograd.grad(a, [x, dec.weight, dec.bias])
        b = torch_rec_loss(x, f, dec)
        gb = torch.autograd.grad(b, [x, dec.weight, dec.bias])
        assert torch.equal(a, b) and all(torch.equal(p, q) for p, q in zip(ga, gb))
    with pytest.raises(RuntimeError):
        capi.rec_loss(code, feats, weight, bias)                                       # the native call itself has no CPU path

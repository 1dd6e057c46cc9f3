"""CPU, no kernel: the gate of tests/split_cases.py can fail.  The rounding model itself stays inside it; each defect below, injected into the
model, falls outside it -- every one of them accepted by kernel_cases.case_split_precision's "1e-4 of the output scale".  The smallest one
decides that attention_cases.RMS_MARGIN is tight enough: `lo` truncated instead of rounded sits at 1.67 x the model's E_rms (measured: 1.66 at
K = 768, 1.67 at K = 3072; E_max 1.4 .. 1.7 x, inside MAX_MARGIN: the rms gate is the one that rejects it)."""
import pytest
import torch

from tests import split_cases as SC
from tests.kernel_cases import rnd

M = N = 256


@pytest.fixture(scope="module", params=[768, 3072])
def gemm(request):
    K = request.param
    a, b = rnd((M, K), 50).double(), rnd((N, K), 51).double()
    return dict(K=K, a=a, b=b, ref=a @ b.t(), model=SC.prod3(a, b))


def _rejected(what, got, model, ref, rms_only=False):
    with pytest.raises(AssertionError, match="rms error" if rms_only else "what the roundings allow"):
        SC.gate(what, got, model, ref)


def test_split_gate_accepts_the_model(gemm):
    SC.gate("model", gemm["model"], gemm["model"], gemm["ref"])
    er, em = SC.errors(gemm["model"], gemm["ref"])
    # the three-term product of N(0, 1) operands: 4.4e-6 rms at every K (the lo lo term and the rounding of lo, 2^-17.8 per product)
    assert 3.5e-6 < er < 5.5e-6 and em < 1e-5, (er, em)
    # ... and evaluated in fp32 (one fp32 rounding per k term, the worst order) it is the same number: accumulation order is invisible here
    ah, al = SC.split(gemm["a"])
    bh, bl = SC.split(gemm["b"])
    f = lambda t: t.float()
    m32 = (f(al) @ f(bh).t() + f(ah) @ f(bl).t() + f(ah) @ f(bh).t()).double()
    e32 = SC.errors(m32, gemm["ref"])[0]
    assert abs(e32 / er - 1) < 0.05, (e32, er)
    SC.gate("model in fp32", m32, gemm["model"], gemm["ref"])


def test_split_gate_rejects_gemm_defects(gemm):
    a, b, ref, model, K = gemm["a"], gemm["b"], gemm["ref"], gemm["model"], gemm["K"]
    ah, al = SC.split(a)
    bh, bl = SC.split(b)
    # 1. lo truncated instead of rounded: the smallest defect
    tl = lambda x: SC.split(x, rd_lo=SC.bf_trunc)
    got = SC.prod3(a, b, tl, tl)
    ratio = SC.errors(got, ref)[0] / SC.errors(model, ref)[0]
    print(f"  lo truncated, K = {K}: {ratio:.3f} x the model's E_rms")
    assert 1.5 < ratio < 1.85, ratio
    _rejected("lo truncated", got, model, ref, rms_only=True)
    # 2. hi truncated
    th = lambda x: SC.split(x, rd_hi=SC.bf_trunc)
    _rejected("hi truncated", SC.prod3(a, b, th, th), model, ref)
    # 3. one k-value of K in plain bf16
    al1, bl1 = al.clone(), bl.clone()
    al1[:, K // 2], bl1[:, K // 2] = 0.0, 0.0
    _rejected("one k-value in plain bf16", SC.terms3(ah, al1, bh, bl1), model, ref)
    # 4. the lo_a hi_b term dropped on 4 k-values (al enters that term only)
    al4 = al.clone()
    al4[:, 16:20] = 0.0
    _rejected("lo_a hi_b dropped on 4 k-values", SC.terms3(ah, al4, bh, bl), model, ref)
    # 5. one output row in plain bf16
    row = model.clone()
    row[M - 1] = ah[M - 1] @ bh.t()
    _rejected("one output row in plain bf16", row, model, ref)


def test_split_gate_rejects_attention_defects():
    B, Ntok = 1, 290
    x = rnd((Ntok, 2304), 70).double()
    ref, ref_lse = SC.reference_fwd(x, Ntok, SC.SCALE)
    model, lse = SC.model_fwd(x, Ntok, SC.SCALE)
    SC.gate("out", model, model, ref)
    assert float((lse - ref_lse).abs().max()) < SC.LSE_ABS
    # P not split: its hi part alone
    only_hi = lambda p: (SC.bf(p), torch.zeros_like(p))
    _rejected("P not split", SC.model_fwd(x, Ntok, SC.SCALE, split_p=only_hi)[0], model, ref)
    # V lo dropped on the last (ragged) key tile: 34 of the 290 keys
    _rejected("V lo dropped on the last key tile", SC.model_fwd(x, Ntok, SC.SCALE, split_v_last=only_hi)[0], model, ref)
    # ... and the backward's gate: dS not split on the way to dK / dQ
    dout = rnd((Ntok, 768), 71).double()
    o, l, g = SC.reference(x, dout, Ntok, SC.SCALE)
    fed = (o.float().double(), l.float().double())
    mb = SC.model_bwd(x, *fed, dout, Ntok, SC.SCALE)
    for name, sl in (("dQ", slice(0, 768)), ("dK", slice(768, 1536)), ("dV", slice(1536, 2304))):
        SC.gate(name, mb[:, sl], mb[:, sl], g[:, sl])
    tl = lambda t: SC.split(t, rd_lo=SC.bf_trunc)
    bad = SC.model_bwd(x, *fed, dout, Ntok, SC.SCALE, sp=tl)
    for name, sl in (("dQ", slice(0, 768)), ("dK", slice(768, 1536)), ("dV", slice(1536, 2304))):
        _rejected(name, bad[:, sl], mb[:, sl], g[:, sl])

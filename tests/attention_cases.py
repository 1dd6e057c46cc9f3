"""The 16-bit attention kernels against what their roundings allow (a sibling of kernel_cases: the same helpers, the same two builds).

case_attention accepts 2e-2 / 3e-2 absolute on results whose rms is 0.07 .. 0.10: gradients off by 5 %, truncated probabilities and a
softmax scale off by 2 % pass it.  Here every 16-bit form is measured against an fp64 REFERENCE (softmax attention and its autograd on
the 16-bit-rounded operands) next to an fp64 MODEL of the flash pipeline that rounds where the kernel under test rounds and nowhere else:

    E_rms = rms(x - ref) / rms(ref),  E_max = max |x - ref| / max |ref|           per tensor (out, dQ, dK, dV)
    gate:   E_rms(kernel) <= 1.25 E_rms(model)   and   E_max(kernel) <= 2 E_max(model)

The margin is for what the model leaves out -- fp32 accumulation order and v_exp_f32, both at 1e-6, three orders below the 16-bit
roundings -- and for the sampling noise of a maximum over a few hundred thousand elements; the smallest defect of
test_attention_gate_rejects_defects (probabilities truncated instead of rounded) sits at 1.5 x rms on `out`.

The model's rounding points, each with the source line that performs it (rd() = lp() then f32(): the calling thread's build):
  shared, forward    P before P V               common.h acc_to_chunk<bf16_t> (pack_bf2), through attention.hip mma_transposed /
                                                mma_transposed_swz; attn_fwd_pw.hip pw_sm_fin (v_cvt_pk)
                     out on store               attn_common.h store_32d_rows16 (pack_bf2), from attention.hip store_dT_ok and the
                                                read-out of attn_fwd_pw.hip (PW_STORE)
  shared, backward   P before P^T dO            common.h acc_to_chunk<bf16_t>, through mma_transposed(_swz)(dv, ..., s)
                     dS before dS^T Q, dS K     the same (dk, ..., dp; dq, ..., dp); attention.hip attn_bwd_fused2/3_kernel `w[0] = key_ok ?
                                                pack_bf2(dp ...` (the exchange tile dQ is computed from: the same value, the same rounding)
                     dqkv on store              attn_common.h store_32d_rows16 (dQ; dK / dV of the two-kernel forms), attention.hip
                                                attn_bwd_fused2/3_kernel `w[0] = pack_bf2(a[4 * g] * m ...` (dK / dV through the LDS patch)
  persistent forward q' = 16-bit(c2 * q), raw q attn_fwd_pw.hip pw_scale_chunk (pack_bf2(lo16f(raw) * c2, ...)); under q_prescaled the rows
                                                are read as they stand (q_take_qs): the single rounding of q' is the operand's own
The probabilities are rounded relative to the running maximum each form keeps: the tile-by-tile maximum of the four-wave forms
(attention.hip attn_fwd_kernel `m_new = fmaxf(m_run, mx * c2)`: a row's largest probability of a tile is exactly 1), the deferred one of
the persistent form (attn_fwd_pw.hip pw_region_slots: m = 0 from the item's start, moved only when a half-row sum of a 32-query block leaves
[PW_COLD, PW_HOT] -- so the largest probability is rounded like any other, which alone is 6 - 14 % of E_rms at these row lengths; the
model asserts that no sum of its inputs leaves that window and keeps m = 0).  The row sum `l` is
that of the UNROUNDED probabilities in every form (attention.hip `ps += pv`; attn_fwd_pw.hip pw_sm_fin adds the exponentials, then
converts them): the persistent form's lse differs from the others' by its second rounding of q' only.
The backward takes the out / lse it is handed; delta = rowsum(dO * O) is an fp32 sum of 16-bit operands (attn_delta_kernel): no rounding.
"""
import math
from functools import partial

import numpy as np
import torch

from maest_amd import _lib, ops
from tests.kernel_cases import f16_build, f32, lp, rnd

H, HD, E = 12, 64, 768
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
PW_HOT, PW_COLD = 4096.0, 1.0e-30   # attn_fwd_pw.hip
RMS_MARGIN, MAX_MARGIN = 1.25, 2.0
LSE_ABS = 1e-5                      # forms that sum unrounded p against an unrounded q: 20 fp32 ulps at |lse| ~ 5


def rd(t):
    """fp64 -> the values the calling thread's build keeps in 16 bits (through fp32, as the kernels convert), as fp64."""
    return f32(lp(t.float())).double()


def truncate(t):
    """fp64 -> 16 bits by dropping the low bits instead of rounding to nearest (a defect: never what a kernel may do)."""
    if f16_build():
        h = t.float().half()
        over = h.float().abs() > t.float().abs()
        down = (h.view(torch.int16) - 1).view(torch.float16)        # (sign-magnitude: one step towards zero)
        return torch.where(over, down, h).double()
    return (t.float().view(torch.int32) & -65536).view(torch.float32).double()


def _heads(t, N):
    """[N, cols * 768] -> [cols, 12, N, 64]"""
    return t.reshape(N, -1, H, HD).permute(1, 2, 0, 3)


def _rows(t, N):
    """[12, N, 64] -> [N, 768]"""
    return t.transpose(0, 1).reshape(N, E)


def _f32mul(a, b):
    return float(np.float32(a) * np.float32(b))


def reference(x, dout, N, scale):
    """fp64 softmax attention of ONE clip and its autograd: x [N, 2304] (the true q, k, v), dout [N, 768] or None
    -> out [N, 768], lse [12, N], dqkv [N, 2304] (None without dout)."""
    x = x.clone().requires_grad_(dout is not None)
    q, k, v = _heads(x, N)
    s = (q @ k.transpose(-2, -1)) * scale
    out = _rows(s.softmax(-1) @ v, N)
    lse = torch.logsumexp(s, -1)
    if dout is None:
        return out.detach(), lse.detach(), None
    out.backward(dout)
    return out.detach(), lse.detach(), x.grad


def model_fwd(xk, N, scale, persistent=False, q_prescaled=False, rd_p=rd):
    """The forward pipeline of ONE clip in fp64 with the roundings of the form: xk [N, 2304] fp64 = the operand the kernel reads (its q
    columns hold q' under q_prescaled).  -> out [N, 768] (16-bit values), lse [12, N].  rd_p: the conversion of P (tests of the gate)."""
    q, k, v = _heads(xk, N)
    c2 = 1.0 if q_prescaled else _f32mul(scale, LOG2E)           # attn_common.h attn_scale
    if persistent and not q_prescaled:
        s2 = lp(q.float() * np.float32(c2))                     # attn_fwd_pw.hip pw_scale_chunk: an fp32 product, rounded
        s2 = f32(s2).double() @ k.transpose(-2, -1)
    else:
        s2 = (q @ k.transpose(-2, -1)) * c2
    nt = (N + 63) // 64
    pad = torch.full((H, N, nt * 64 - N), -math.inf, dtype=torch.float64)
    st = torch.cat([s2, pad], -1).reshape(H, N, nt, 64)
    tmax = st.amax(-1)                                           # [12, N, nt]
    if not persistent:
        mrun = torch.cummax(tmax, -1).values
    else:
        # attn_fwd_pw.hip pw_region_slots: an item starts at m = 0 and keeps it -- P = 2^S' as it stands, the largest probability of a
        # row rounded like every other -- as long as every half-row sum of a tile (common.h frag_row: the keys of a lane's half-wave)
        # stays inside [PW_COLD, PW_HOT] (the first tile; later ones: below PW_HOT).  The model covers that path only and says so: the
        # kernel's rescale path (pw_softmax_slow) is case_attention_exact's, with `hot`
        half = ((torch.arange(64) >> 2) & 1).bool()
        e = torch.exp2(st)
        h0, h1 = e[..., ~half].sum(-1), e[..., half].sum(-1)
        assert bool((h0 <= PW_HOT).all() and (h1 <= PW_HOT).all() and (h0[..., 0] >= PW_COLD).all() and (h1[..., 0] >= PW_COLD).all()), \
            "a half-row sum leaves [PW_COLD, PW_HOT]: the persistent form would rescale, which this model does not follow"
        mrun = torch.zeros_like(tmax)
    mfin = mrun[..., -1]
    p = torch.exp2(st - mrun[..., None])                         # against the maximum known when the tile is processed
    w = torch.exp2(mrun - mfin[..., None])[..., None]            # the rescaling that follows: exact factors of the fp32 state
    l = (p * w).reshape(H, N, -1).sum(-1)
    pr = (rd_p(p) * w).reshape(H, N, -1)[..., :N]
    out = rd(_rows((pr @ v) / l[..., None], N))
    return out, (mfin + torch.log2(l)) * LN2


def model_bwd(xk, out, lse, dout, N, scale, q_prescaled=False, delta=None):
    """The backward pipeline of ONE clip in fp64 with the kernels' roundings, on the out / lse it is handed (fp64 values of the tensors
    the kernel reads).  -> dqkv [N, 2304] (16-bit values); dQ is the gradient with respect to the true q in either contract."""
    q, k, v = _heads(xk, N)
    do, o = _heads(dout, N)[0], _heads(out, N)[0]
    c2, s_dq, s_dk = (1.0, scale, LN2) if q_prescaled else (_f32mul(scale, LOG2E), scale, scale)
    if delta is None:
        delta = (do * o).sum(-1)
    p = torch.exp2((q @ k.transpose(-2, -1)) * c2 - (lse * LOG2E)[..., None])
    ds = p * (do @ v.transpose(-2, -1) - delta[..., None])
    dv = rd(p).transpose(-2, -1) @ do
    dk = (rd(ds).transpose(-2, -1) @ q) * s_dk
    dq = (rd(ds) @ k) * s_dq
    return rd(torch.cat([_rows(dq, N), _rows(dk, N), _rows(dv, N)], 1))


def errors(x, ref):
    """(E_rms, E_max) of x against ref."""
    d = x.double() - ref
    return (float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max() / ref.abs().max()))


def gate(what, got, model, ref, ratios=None):
    """Require E_rms(got) <= 1.25 E_rms(model) and E_max(got) <= 2 E_max(model); print and record the two ratios."""
    (gr, gm), (mr, mm) = errors(got, ref), errors(model, ref)
    assert mr > 0 and mm > 0, f"{what}: the model shows no rounding error: nothing to compare with"
    print(f"  {what}: E_rms {gr:.3e} = {gr / mr:.3f} x model ({mr:.3e}), E_max {gm:.3e} = {gm / mm:.3f} x model ({mm:.3e})")
    if ratios is not None:
        key = what.split(":")[0]
        ratios[key] = (max(ratios.get(key, (0, 0))[0], gr / mr), max(ratios.get(key, (0, 0))[1], gm / mm))
    assert gr <= RMS_MARGIN * mr, f"{what}: rms error {gr:.3e} is {gr / mr:.2f} x what the roundings allow ({mr:.3e})"
    assert gm <= MAX_MARGIN * mm, f"{what}: max error {gm:.3e} is {gm / mm:.2f} x what the roundings allow ({mm:.3e})"


def gate_dqkv(what, got, model, ref, ratios=None):
    for name, sl in (("dQ", slice(0, E)), ("dK", slice(E, 2 * E)), ("dV", slice(2 * E, 3 * E))):
        gate(f"{what}: {name}", got[:, sl], model[:, sl], ref[:, sl], ratios)


def _clip(t, b, N):
    return f32(t[b * N:(b + 1) * N].detach().cpu()).double()


def _fwd_forms(N, restricted):
    """(name, ops.options, persistent kernel, feeds the backward) of every 16-bit forward form serving the shape.  On the host emulator,
    which takes seconds per launch: not the other workgroup sizes of the four-wave form, and the four-wave LDS-DMA form once -- as the
    default, which it is up to 320 tokens (attention.hip attn_fwd_launch), not a second time by its option."""
    emu = _lib.host_emulation()
    pw_default = N > 320 and not restricted
    forms = [("default", {}, pw_default, restricted or (emu and not pw_default)), ("register-staged tiles", {"attn_fwd": 1}, False, False)]
    if not emu or pw_default:
        forms.append(("four-wave, LDS-DMA tiles", {"attn_fwd": 2}, False, not restricted))
    if not restricted:
        forms.append(("persistent", {"attn_fwd": 3}, True, True))
    if not emu:
        forms += [(f"{nw} waves per workgroup", {"attn_fwd": 2, "attn_fwd_waves": nw}, False, False) for nw in (5, 6, 8)]
    return forms


def _bwd_forms(N, restricted):
    """(name, ops.options) of every backward form serving the shape: the default (fused below 320 tokens -- persistent from 257 --, two-kernel
    LDS-DMA above), the two-kernel form where it is not the default, the per-item fused one where the default is the persistent one, and
    the register-staged two-kernel form (bit-equal to the DMA-fed one, case_attention: on the device only)."""
    forms = [("default", {})]
    if restricted:
        return forms          # (attention.hip attn_bwd_launch: q_rows < N always takes attn_bwd_fused2_kernel, with attn_bwd = 3 as well)
    if N <= 320:
        forms.append(("two-kernel, LDS-DMA tiles", {"attn_bwd": 1}))
    if 256 < N <= 320:
        forms.append(("fused, one workgroup per item", {"attn_bwd": 3}))
    if not _lib.host_emulation():
        forms.append(("two-kernel, register-staged tiles", {"attn_bwd": 4}))
    return forms


def case_attention_calibrated(dev, B, N, qs=False, q_rows=None, seed=20):
    """Every 16-bit forward and backward form at [B, N] through gate() against the fp64 reference and the rounding model of its form, in
    the calling thread's build.  The backward forms are fed the reference's out / lse (rounded to 16 bits) and the out / lse of the
    four-wave LDS-DMA and of the persistent forward.  qs: the MAEST_BF16_QS contract (case_attention).  q_rows: the restricted forward's rows and
    the restricted fused backward, against the model fed a dO that is zero beyond row q_rows.  B > 3: the kernels run on the whole batch,
    the first, a middle and the last clip are compared.  Returns {form: (worst rms ratio, worst max ratio)}."""
    scale, c = 0.125, 0.125 * LOG2E
    restricted = q_rows is not None
    qkv = lp(rnd((B * N, 2304), seed, 1.0))
    x = f32(qkv).double()                                        # the reference's operand: the true q
    if qs:
        qp = lp(f32(qkv[:, :E]) * c)                             # what the row-scaled projection writes
        qkv = torch.cat([qp, qkv[:, E:]], 1).contiguous()
        x = torch.cat([f32(qp).double() / c, x[:, E:]], 1)
    xk = f32(qkv).double()                                       # the kernels' operand
    dout = f32(lp(rnd((B * N, E), seed + 1))).reshape(B, N, E)
    nv = N if not restricted else min(32, N)                     # rows the forward writes
    if restricted:
        dout[:, q_rows:] = 0.0
    dout = lp(dout.reshape(B * N, E))
    clips = sorted({0, B // 2, B - 1})
    pick = lambda t: torch.cat([_clip(t, b, N)[:nv] if t.shape[1] == E else _clip(t, b, N) for b in clips])
    pick_lse = lambda t: torch.cat([t[b].detach().cpu().double()[:, :nv] for b in clips])
    # reference: forward of every clip (the backward is fed it), autograd of the compared ones
    ref_out, ref_lse, ref_g = [], [], {}
    for b in range(B):
        o, l, g = reference(x[b * N:(b + 1) * N], f32(dout[b * N:(b + 1) * N]).double() if b in clips else None, N, scale)
        ref_out.append(o), ref_lse.append(l)
        if b in clips:
            ref_g[b] = g
    ref_out, ref_lse = torch.cat(ref_out), torch.stack(ref_lse)
    ref_g = torch.cat([ref_g[b] for b in clips])
    ratios = {}
    attn_fwd, attn_bwd = partial(ops.attn_fwd, q_prescaled=qs), partial(ops.attn_bwd, q_prescaled=qs)
    kq = {} if not restricted else {"q_rows": q_rows}
    print(f"attention against its rounding model, {'f16' if f16_build() else 'bf16'} build, B = {B}, N = {N}, qs = {qs}, q_rows = {q_rows}")
    # ---- forward
    models = {}
    for pers in (False, True):
        mo = [model_fwd(xk[b * N:(b + 1) * N], N, scale, pers, qs) for b in clips]
        models[pers] = (torch.cat([o[:nv] for o, _ in mo]), torch.cat([l[:, :nv] for _, l in mo]))
    r_out, r_lse = pick(ref_out), pick_lse(ref_lse)
    lse_model_err = float((models[True][1] - r_lse).abs().max())
    fed = {}
    for name, opt, pers, feeds in _fwd_forms(N, restricted):
        with ops.options(**opt):
            out, lse = attn_fwd(qkv.to(dev), B, N, scale, save_lse=True, **kq)
        gate(f"forward ({name}): out", pick(out), models[pers][0], r_out, ratios)
        el = float((pick_lse(lse) - r_lse).abs().max())
        # (the persistent form: twice what its second rounding of q' does to the model's lse; with q' handed over -- qs -- it rounds
        # nothing on the way to lse and belongs with the forms that sum unrounded p)
        lim = max(2 * lse_model_err, LSE_ABS) if pers else LSE_ABS
        print(f"  forward ({name}): lse within {el:.2e} of the reference (limit {lim:.2e})")
        assert el <= lim, f"forward ({name}): lse {el:.3e} from the reference, limit {lim:.3e}"
        if feeds:
            fed[f"the {name} forward"] = (out, lse)
    # ---- backward: every form on the reference's out / lse and on its own forwards'
    fed = {"the reference": (lp(ref_out.float()).to(dev), ref_lse.float().contiguous().to(dev)), **fed}
    if restricted and not ops.attn_bwd_rows_supported(torch.bfloat16, N):
        return ratios
    for src, (o, l) in fed.items():
        o64, l64 = f32(o.cpu()).double().reshape(B, N, E).clone(), l.cpu().double().clone()
        o64[:, nv:], l64[:, :, nv:] = 0.0, 0.0                   # (rows a restricted forward leaves unwritten: never read, dO = 0 there)
        mg = torch.cat([model_bwd(xk[b * N:(b + 1) * N], o64[b], l64[b], f32(dout[b * N:(b + 1) * N]).double(), N, scale, qs) for b in clips])
        for name, opt in _bwd_forms(N, restricted):
            with ops.options(**opt):
                dqkv = attn_bwd(qkv.to(dev), o, dout.to(dev), l, B, N, scale, **kq)
            gate_dqkv(f"backward ({name}) on the out / lse of {src}", torch.cat([_clip(dqkv, b, N) for b in clips]), mg, ref_g, ratios)
    return ratios


# ------------------------------------------------------------------------------ a forward whose answer is known exactly
def exact_inputs(B, N, seed=40, hot=False):
    """q one-hot at class c = i % 64; k[j, c] = the score in log2 units of query class c on key j: 0 where (j + 7 c) % 32 == 0, else
    -10 - ((j + c) % 4), and +6 at key (N - 1 - c) % N (one late maximum per class: the rescale path), rolled by the head index along c;
    v integers in [-4, 4].  Every value is exact in bf16 and in half.  -> qkv fp32 [B * N, 2304], the scores [12, N, N] and v [B, 12, N, 64].
    hot: the levels that send the persistent forward down its rescale path (attn_fwd_pw.hip pw_softmax_slow), which no softmax of random
    scores reaches: the late maximum is +13 (a half-row sum of 2^13 > PW_HOT: m is raised on a later tile; where that key lies in the
    first tile, m is set there) over a background of -8 - ((j + c) % 4) (so that 2^(-11 - 13) is still a half value), and for the classes
    c % 16 == 5 every key of the upper half-wave's share of the first tile (frag_row: key & 4) sits at -110: that half-row sums to
    2^-105 < PW_COLD."""
    j, cc = torch.arange(N)[:, None], torch.arange(64)[None, :]
    lev = torch.where((j + 7 * cc) % 32 == 0, 0.0, (-8.0 if hot else -10.0) - ((j + cc) % 4).float())
    if hot:
        lev = torch.where((j < 64) & ((j & 4) != 0) & (cc % 16 == 5), -110.0, lev)
    lev[(N - 1 - torch.arange(64)) % N, torch.arange(64)] = 13.0 if hot else 6.0
    k = torch.stack([torch.roll(lev, h, 1) for h in range(H)], 1)               # [N, 12, 64]
    q = torch.zeros(N, H, 64)
    q[torch.arange(N), :, torch.arange(N) % 64] = 1.0
    rng = np.random.Generator(np.random.PCG64(seed))
    v = torch.from_numpy(rng.integers(-4, 5, (B, N, H, 64)).astype(np.float32))
    qkv = torch.cat([q.reshape(1, N, E).expand(B, N, E), k.reshape(1, N, E).expand(B, N, E), v.reshape(B, N, E)], 2).reshape(B * N, 2304)
    s = k.permute(1, 0, 2)[:, :, torch.arange(N) % 64].transpose(1, 2).double()  # [12, i, j] = k[j, h, c(i)]
    return qkv.contiguous(), s, v.permute(0, 2, 1, 3).double()


def exact_reference(s, v, drop_key=None):
    """fp64 sum 2^(s - m) v / sum 2^(s - m) and lse = (m + log2 l) ln 2: every term a power of two.  -> out [B, N, 768], lse [12, N].
    drop_key: leave one key out (tests of the gate)."""
    if drop_key is not None:
        keep = torch.arange(s.shape[-1]) != drop_key
        s, v = s[..., keep], v[:, :, keep]
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.sum(-1)
    out = (p @ v) / l[..., None]                                               # [B, 12, N, 64]
    return out.transpose(1, 2).reshape(v.shape[0], -1, E), (m[..., 0] + torch.log2(l)) * LN2


def ulp16(ref):
    """One ulp of the calling thread's 16-bit format at |ref|, as the issue counts it: 2^-8 (bf16) / 2^-11 (half) of the value -- the
    largest distance a correctly rounded normal result can have -- and the format's smallest step below that (half: 2^-24; the
    weighted sums of small integers cancel down to 1e-9 on a few elements)."""
    return torch.clamp(ref.abs() * 2.0 ** -11, min=2.0 ** -24) if f16_build() else torch.clamp(ref.abs() * 2.0 ** -8, min=2.0 ** -133)


def exact_gate(what, out, lse, ref_out, ref_lse):
    """out (fp64 values of the 16-bit result) within one ulp of the reference, lse within 1e-5; prints the share bit-equal to the rounded reference."""
    err = (out - ref_out).abs()
    bad = err > ulp16(ref_out)
    same = float((out == rd(ref_out)).double().mean())
    el = float((lse - ref_lse).abs().max())
    print(f"  {what}: {100 * same:.2f} % of out bit-equal to the rounded reference, {int(bad.sum())} beyond one ulp, lse within {el:.1e}")
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} elements beyond one ulp of the exact answer; first at "
                                 f"{tuple(int(i) for i in bad.nonzero()[0])}")
    assert el <= LSE_ABS, f"{what}: lse {el:.3e} from the exact answer"


def case_attention_exact(dev, B, N, qs=False, hot=False):
    """Every forward form (the workgroup sizes and the restricted rows included) on exact_inputs: a misplaced, dropped or doubled key, a wrong tail
    mask, a rescale applied twice or a stale ring slot moves thousands of elements past one ulp, which no random softmax shows.
    qs: the q columns hold the scores' factor directly (q_prescaled); raw q: scale = ln 2, so that scale * log2(e) is 1.
    hot: exact_inputs' levels for the persistent form's rescale path (first tile below PW_COLD, a later one above PW_HOT)."""
    qkv32, s, v = exact_inputs(B, N, hot=hot)
    ref_out, ref_lse = exact_reference(s, v)
    qkv = lp(qkv32)
    assert torch.equal(f32(qkv), qkv32), "the construction must be exact in 16 bits"
    scale = 0.125 if qs else LN2
    print(f"attention forward with an exactly known answer, {'f16' if f16_build() else 'bf16'} build, B = {B}, N = {N}, qs = {qs}, hot = {hot}")
    for restricted in (False, True):
        nv = min(32, N) if restricted else N
        for name, opt, _, _ in _fwd_forms(N, restricted):
            with ops.options(**opt):
                out, lse = ops.attn_fwd(qkv.to(dev), B, N, scale, save_lse=True, q_prescaled=qs, **({"q_rows": 2} if restricted else {}))
            out = f32(out.cpu()).double().reshape(B, N, E)[:, :nv]
            lse = lse.cpu().double()[:, :, :nv]
            exact_gate(f"{name}{', rows of the first tile only' if restricted else ''}", out, lse, ref_out[:, :nv], ref_lse[None, :, :nv].expand(B, H, nv))

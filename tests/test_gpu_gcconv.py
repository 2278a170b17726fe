"""Gated carried convolution plans on the GPU (tfft_gcconv_*, include/tfft_gcconv.h): the gated overlap-save causal convolution and
its gradients on a chunk of a longer sequence, the history in front of x AND of the pre gate and the future behind gy AND of the post
gate read from pointers of their own.

The kernels are the shipped gated ones with their load ends re-indexed, and every window they transform is a window the shipped gated
plans transform on a concatenated sequence (tests/gcconv_ref.py, checked in numpy by tests/test_gcconv_host.py). So the reference is
shipped, validated code, BIT FOR BIT:

  1. forward: samples [hop, hop + L) of TfftGatedLongConvPlan at length hop + L on [zeros | hist | x], [ones | pre_hist | pre],
     [ones | post] (the gate padding is +1: the -0 trap of tests/gcconv_ref.py),
  2. input gradient: samples [0, L) of TfftGatedLongConvGradPlan at length L + Fn on [gy | fut], [post | post_fut], [x | ones],
     [pre | ones]: dx and dpre,
  3. tap gradient: with partials = 1 on both sides the bits of that plan at length hop + L on the front-padded sequences; with
     partials 0 and 2 within dh_bound of the fp64 sum over the plan's own items, two executions the same bits, dskip the bits of
     dh[:, 0],
  4. a plan without gates and skip: libtfft_cconv.so's bits; NULL contexts: libtfft_gsconv.so's / libtfft_gbconv.so's bits,
  5. three chunks out of one buffer that x and pre share: the whole-sequence gated plans' y, dx and dpre,
  6. the contract: which context pointers go together, aliasing, launch_iters, stream capture, every instantiation launched,
  7. autograd over two chunks against fp64 torch.autograd of the whole operator, 8. strided views, 9. the example.

Every execution of 1 - 4 runs between NaN-filled guard zones; sequences, gates and contexts have padded, unequal strides whose gaps
hold NaN bit patterns, so a read outside [0, L) of a sequence or gate or [0, Hn) / [0, Fn) of a context poisons the result.
No tolerance constant of its own: K_SCONV, dh_bound and the derived gate tolerances of tests/gsconv_ref.py and tests/gbconv_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import bconv_ref as br
import cconv_ref as cr
import dist_emulate as de
import elementwise_bound as eb
import gbconv_ref as gb
import gcconv_ref as gc
import gsconv_ref as gs
import sconv_ref as sr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# the sequence strides of the guarded executions: unequal, so that a stride taken from the wrong tensor shows
PAD = dict(x=8, pre=40, post=56, gy=24, out=24, dpre=72, hist=16, pre_hist=32, fut=16, post_fut=48)


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and not np.isnan(a.astype(np.float32)).any() and np.array_equal(_bits(a), _bits(b))


def _inst(pre, post):
    return f"<{'true' if pre else 'false'}, {'true' if post else 'false'}>"


def fwd_kernels(pre, post):
    return ["gcconv4096::fwd_kernel" + _inst(pre, post)]


def grad_kernels(pre, post):
    return ["gcconv4096::dgrad_kernel" + _inst(pre, post), "gcconv4096::wgrad_kernel" + _inst(pre, post), "gcconv4096::wreduce_kernel"]


class Seqs:
    """[B][C][n] binary16 on the device between guard zones, sequence s at s * stride, gaps and guards NaN (tests/test_gpu_cconv.py)"""

    def __init__(self, x, pad):
        self.shape = x.shape
        seqs, n = x.shape[0] * x.shape[1], x.shape[2]
        self.stride = n + pad
        self.host = np.full((seqs - 1) * self.stride + n, de.SENTINEL, dtype=np.int16)
        self.idx = (np.arange(seqs) * self.stride)[:, None] + np.arange(n)[None, :]
        self.host[self.idx] = np.ascontiguousarray(x).reshape(seqs, n).view(np.int16)
        self.buf = de._guarded(torch, self.host.size, self.host.view(np.float16))
        self.flat = self.buf[de.GUARD:de.GUARD + self.host.size]

    def untouched(self, what):
        assert de._guards_intact(torch, self.buf), what
        de._untouched(self.flat.cpu().numpy().view(np.int16), self.host, what)


class Out:
    """an output of [B][C][L] binary16 between guard zones, all sentinels before the execution"""

    def __init__(self, shape, pad):
        self.shape, seqs = shape, shape[0] * shape[1]
        self.stride = shape[2] + pad
        self.n = (seqs - 1) * self.stride + shape[2]
        self.idx = (np.arange(seqs) * self.stride)[:, None] + np.arange(shape[2])[None, :]
        self.buf = de._guarded(torch, self.n)
        self.flat = self.buf[de.GUARD:de.GUARD + self.n]

    def result(self):
        assert de._guards_intact(torch, self.buf), "output guard zone written"
        out = self.flat.cpu().numpy().view(np.int16)
        gaps = np.ones(self.n, bool)
        gaps[self.idx.reshape(-1)] = False
        assert (out[gaps] == de.SENTINEL).all(), "halves between output sequences written"
        return out[self.idx].view(np.float16).reshape(self.shape)


def _dev(a):
    """a flat device copy, or None (the shared case data is read-only on the host)"""
    return None if a is None else torch.from_numpy(np.array(a).reshape(-1)).to(DEV)


def _seqs(d, names):
    return {k: (Seqs(d[k], PAD[k]) if d.get(k) is not None else None) for k in names}


def _flat(s):
    return None if s is None else s.flat


def _stride(s):
    return 0 if s is None else s.stride


def _untouched(s):
    for k, v in s.items():
        if v is not None:
            v.untouched(k)


def run_fwd(tf, d, launch_iters=0, room=None):
    """one carried forward execution of the case dict d; room: the plan's Hn where d has no history (a NULL history on a plan that has
    room for one)"""
    rows, channels, length = d["x"].shape
    taps = d["h"].shape[1]
    hn = d["hist"].shape[2] if d["hist"] is not None else (room or 0)
    s = _seqs(d, ("x", "pre", "post", "hist", "pre_hist"))
    out = Out(d["x"].shape, PAD["out"])
    has = (d["pre"] is not None, d["post"] is not None)
    plan = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, pre_gate=has[0], post_gate=has[1], in_seq_stride=s["x"].stride,
                                       out_seq_stride=out.stride, pre_seq_stride=_stride(s["pre"]), post_seq_stride=_stride(s["post"]),
                                       launch_iters=launch_iters, history=hn, hist_seq_stride=_stride(s["hist"]),
                                       pre_hist_seq_stride=_stride(s["pre_hist"]))
    assert (plan.halo, plan.hop, plan.segments) == sr.geometry(length, taps) and plan.carry_min == gc.carry_min(taps)
    assert plan.num_launches == 1 and plan.kernels == fwd_kernels(*has)
    plan.set_taps(_dev(d["h"]), _dev(d["skip"]))
    plan.exec(s["x"].flat, out.flat, pre=_flat(s["pre"]), post=_flat(s["post"]), hist=_flat(s["hist"]), pre_hist=_flat(s["pre_hist"]))
    torch.cuda.synchronize()
    y = out.result()
    _untouched(s)
    plan.close()
    return y


def run_dx(tf, d, launch_iters=0, room=None, want_dpre=True):
    """one carried input gradient: (dx, dpre or None)"""
    rows, channels, length = d["gy"].shape
    taps = d["h"].shape[1]
    fn = d["fut"].shape[2] if d["fut"] is not None else (room or 0)
    has = (d["pre"] is not None, d["post"] is not None)
    s = _seqs(d, ("gy", "post", "fut", "post_fut") + (("x", "pre") if has[0] else ()))
    dx = Out(d["gy"].shape, PAD["out"])
    dpre = Out(d["gy"].shape, PAD["dpre"]) if has[0] and want_dpre else None
    plan = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, pre_gate=has[0], post_gate=has[1], gy_seq_stride=s["gy"].stride,
                                           post_seq_stride=_stride(s["post"]), x_seq_stride=_stride(s.get("x")), pre_seq_stride=_stride(s.get("pre")),
                                           dx_seq_stride=dx.stride, dpre_seq_stride=dpre.stride if dpre else 0, launch_iters=launch_iters, future=fn,
                                           fut_seq_stride=_stride(s["fut"]), post_fut_seq_stride=_stride(s["post_fut"]))
    assert plan.num_launches == 3 and plan.kernels == grad_kernels(*has)
    plan.set_taps(_dev(d["h"]), _dev(d["skip"]))
    plan.input_grad(s["gy"].flat, dx.flat, post=_flat(s["post"]), x=_flat(s.get("x")), pre=_flat(s.get("pre")), dpre=None if dpre is None else dpre.flat,
                    future=_flat(s["fut"]), post_future=_flat(s["post_fut"]))
    torch.cuda.synchronize()
    res = dx.result(), (None if dpre is None else dpre.result())
    _untouched(s)
    plan.close()
    return res


def run_dh(tf, d, partials=0, room=None, twice=False):
    """one (or two) carried tap gradients: (dh [C][K], dskip [C]) fp32 between guard words"""
    rows, channels, length = d["x"].shape
    taps = d["h"].shape[1]
    hn = d["hist"].shape[2] if d["hist"] is not None else (room or 0)
    has = (d["pre"] is not None, d["post"] is not None)
    s = _seqs(d, ("x", "pre", "gy", "post", "hist", "pre_hist"))
    plan = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, pre_gate=has[0], post_gate=has[1], x_seq_stride=s["x"].stride,
                                           pre_seq_stride=_stride(s["pre"]), gy_seq_stride=s["gy"].stride, post_seq_stride=_stride(s["post"]),
                                           partials=partials, history=hn, hist_seq_stride=_stride(s["hist"]),
                                           pre_hist_seq_stride=_stride(s["pre_hist"]))
    assert plan.partials == br.partials_of(rows, channels, length, taps, partials) and plan.kernels == grad_kernels(*has)
    outs = []
    for _ in range(2 if twice else 1):
        buf = torch.full((64 + channels * taps + 64 + channels + 64,), float("nan"), dtype=torch.float32, device=DEV)
        dh, dskip = buf[64:64 + channels * taps], buf[128 + channels * taps:128 + channels * taps + channels]
        plan.tap_grad(s["x"].flat, s["gy"].flat, dh, pre=_flat(s["pre"]), post=_flat(s["post"]), dskip=dskip, history=_flat(s["hist"]),
                      pre_history=_flat(s["pre_hist"]))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        keep = np.ones(host.size, bool)
        keep[64:64 + channels * taps] = False
        keep[128 + channels * taps:128 + channels * taps + channels] = False
        assert np.isnan(host[keep]).all(), "tap or skip gradient written outside [C][K] / [C]"
        outs.append((host[64:64 + channels * taps].reshape(channels, taps).copy(), host[128 + channels * taps:128 + channels * taps + channels].copy()))
    _untouched(s)
    plan.close()
    return outs if twice else outs[0]


# ---- the shipped gated plans on dense sequences

def long_fwd(tf, x, h, pre, post, skip):
    rows, channels, length = x.shape
    plan = tf.TfftGatedLongConvPlan(rows, channels, length, h.shape[1], 0, pre_gate=pre is not None, post_gate=post is not None)
    plan.set_taps(_dev(h), _dev(skip))
    d_y = torch.zeros(x.size, dtype=torch.float16, device=DEV)
    plan.exec(_dev(x), d_y, pre=_dev(pre), post=_dev(post))
    torch.cuda.synchronize()
    plan.close()
    return d_y.cpu().numpy().reshape(x.shape)


def long_dx(tf, gy, h, post, x, pre, skip):
    rows, channels, length = gy.shape
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, h.shape[1], 0, pre_gate=pre is not None, post_gate=post is not None)
    plan.set_taps(_dev(h), _dev(skip))
    d_dx = torch.zeros(gy.size, dtype=torch.float16, device=DEV)
    d_dpre = torch.zeros_like(d_dx) if pre is not None else None
    plan.input_grad(_dev(gy), d_dx, post=_dev(post), x=_dev(x), pre=_dev(pre), dpre=d_dpre)
    torch.cuda.synchronize()
    plan.close()
    return d_dx.cpu().numpy().reshape(gy.shape), (None if d_dpre is None else d_dpre.cpu().numpy().reshape(gy.shape))


def long_dh(tf, x, pre, gy, post, taps, partials=0):
    rows, channels, length = x.shape
    plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None, partials=partials)
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    dskip = torch.zeros((channels,), dtype=torch.float32, device=DEV)
    plan.tap_grad(_dev(x), _dev(gy), dh, pre=_dev(pre), post=_dev(post), dskip=dskip)
    torch.cuda.synchronize()
    plan.close()
    return dh.cpu().numpy(), dskip.cpu().numpy()


_data_cache = {}


def case(length, taps, rows, channels, ctx, kind, mode, seed=1):
    """the case dict of tests/gcconv_ref.py, computed once and shared (never written)"""
    key = (length, taps, rows, channels, ctx, kind, mode, seed)
    if key not in _data_cache:
        d = gc.case_data(length, taps, rows, channels, ctx, kind, seed, mode)
        for a in d.values():
            if a is not None:
                a.setflags(write=False)
        _data_cache[key] = d
    return _data_cache[key]


def _no_context(d):
    return dict(d, hist=None, pre_hist=None, fut=None, post_fut=None)


def _first_bad(a, b):
    return np.argwhere(_bits(a) != _bits(b))[:3].tolist()


# ------------------------------------------------------------------------------------------- 1. forward

@pytest.mark.parametrize("kind", gc.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters,mode", gc.CASE_MODES)
def test_forward_is_the_shipped_gated_plan_on_the_concatenated_sequences(tf, length, taps, rows, channels, ctx, launch_iters, mode, kind):
    d = case(length, taps, rows, channels, ctx, kind, mode)
    hop = sr.geometry(length, taps)[1]
    y = run_fwd(tf, d, launch_iters)
    cx, cpre, cpost = gc.forward_concat(d, taps)
    want = long_fwd(tf, cx, d["h"], cpre, cpost, d["skip"])[:, :, hop:hop + length]
    assert _same_bits(y, want), f"gcconv L={length} K={taps} Hn={ctx} {mode} {kind}: first differing (b, c, t) = {_first_bad(y, want)}"


# ------------------------------------------------------------------------------------------- 2. input gradient

@pytest.mark.parametrize("kind", gc.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters,mode", gc.CASE_MODES)
def test_input_grad_is_the_shipped_gated_plan_on_the_concatenated_sequences(tf, length, taps, rows, channels, ctx, launch_iters, mode, kind):
    d = case(length, taps, rows, channels, ctx, kind, mode)
    dx, dpre = run_dx(tf, d, launch_iters)
    cgy, cpost, cx, cpre = gc.input_grad_concat(d)
    want_dx, want_dpre = long_dx(tf, cgy, d["h"], cpost, cx, cpre, d["skip"])
    what = f"gcconv dgrad L={length} K={taps} Fn={ctx} {mode} {kind}"
    assert _same_bits(dx, want_dx[:, :, :length]), f"{what}: dx, first differing (b, c, t) = {_first_bad(dx, want_dx[:, :, :length])}"
    assert (dpre is None) == (d["pre"] is None)
    if dpre is not None:
        assert _same_bits(dpre, want_dpre[:, :, :length]), f"{what}: dpre, first differing (b, c, t) = {_first_bad(dpre, want_dpre[:, :, :length])}"
        # dpre = NULL on a plan with a pre gate writes dx only, the same bits
        assert _same_bits(run_dx(tf, d, launch_iters, want_dpre=False)[0], dx), what


# ------------------------------------------------------------------------------------------- 3. tap gradient

@pytest.mark.parametrize("kind", gc.TAP_KINDS)
@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters,mode", gc.CASE_MODES)
def test_tap_grad_is_the_shipped_gated_plan_on_the_concatenated_sequences(tf, length, taps, rows, channels, ctx, launch_iters, mode, kind):
    d = case(length, taps, rows, channels, ctx, kind, mode)
    what = f"gcconv wgrad L={length} K={taps} Hn={ctx} {mode} {kind}"
    # partials = 1 on both sides: the same items in the same order; the extra items of the long plan hold zeros of gz and add exact zeros
    dh1, dskip1 = run_dh(tf, d, partials=1)
    cx, cpre, cgy, cpost = gc.tap_grad_concat(d, taps)
    want, want_skip = long_dh(tf, cx, cpre, cgy, cpost, taps, partials=1)
    assert _same_bits(dh1, want), f"{what}: partials 1 differs from the shipped plan in {(_bits(dh1) != _bits(want)).sum()} taps"
    assert _same_bits(dskip1, want_skip) and np.array_equal(_bits(dskip1), _bits(dh1[:, 0].copy())), what
    # the fp64 sum over the plan's own items, of the rounded products the kernel sees, within dh_bound
    items = gc.dh_items(d, taps)
    ref = br.dh_from_items(items, channels, taps)
    bound = br.dh_bound(items, channels)
    for partials in (0, 2):
        (a, a_skip), (b, b_skip) = run_dh(tf, d, partials=partials, twice=True)
        assert _same_bits(a, b) and _same_bits(a_skip, b_skip), f"{what}: partials {partials}: two executions differ"
        assert np.array_equal(_bits(a_skip), _bits(a[:, 0].copy())), f"{what}: dskip is not dh[:, 0]"
        err = np.abs(a.astype(np.float64) - ref)
        print(f"{what}: partials {partials}: worst {float((err / bound[:, None]).max()):.3f} of dh_bound")
        assert (err <= bound[:, None]).all(), f"{what}: partials {partials}: {float((err / bound[:, None]).max()):.3f} of dh_bound"
    assert (np.abs(dh1.astype(np.float64) - ref) <= bound[:, None]).all(), what


# ------------------------------------------------------------------------------------------- 4. the shipped libraries' bits

def _cconv_results(tf, d):
    """y, dx, dh of libtfft_cconv.so on dense copies"""
    rows, channels, length = d["x"].shape
    taps = d["h"].shape[1]
    ctx = d["hist"].shape[2]
    fwd = tf.TfftChunkedConvPlan(rows, channels, length, taps, 0, history=ctx)
    grad = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, history=ctx, future=ctx)
    fwd.set_taps(_dev(d["h"]))
    grad.set_taps(_dev(d["h"]))
    d_y = torch.zeros(d["x"].size, dtype=torch.float16, device=DEV)
    d_dx = torch.zeros_like(d_y)
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    fwd.exec(_dev(d["x"]), d_y, _dev(d["hist"]))
    grad.input_grad(_dev(d["gy"]), d_dx, _dev(d["fut"]))
    grad.tap_grad(_dev(d["x"]), _dev(d["gy"]), dh, _dev(d["hist"]))
    torch.cuda.synchronize()
    fwd.close()
    grad.close()
    return d_y.cpu().numpy().reshape(d["x"].shape), d_dx.cpu().numpy().reshape(d["x"].shape), dh.cpu().numpy()


@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters", gc.WITH_CONTEXT)
def test_without_gates_and_skip_the_bits_are_the_ungated_carried_plans(tf, length, taps, rows, channels, ctx, launch_iters):
    d = dict(case(length, taps, rows, channels, ctx, "noise", gc.EVERY_CASE_MODE), pre=None, post=None, skip=None, pre_hist=None, post_fut=None)
    want_y, want_dx, want_dh = _cconv_results(tf, d)
    assert _same_bits(run_fwd(tf, d, launch_iters), want_y), "y"
    dx, dpre = run_dx(tf, d, launch_iters)
    assert dpre is None and _same_bits(dx, want_dx), "dx"
    assert _same_bits(run_dh(tf, d)[0], want_dh), "dh"


@pytest.mark.parametrize("length,taps,rows,channels,ctx,launch_iters,mode", gc.CASE_MODES)
def test_null_contexts_give_the_shipped_gated_plans(tf, length, taps, rows, channels, ctx, launch_iters, mode):
    """NULL contexts, on plans created with and without room for them: every bit of libtfft_gsconv.so / libtfft_gbconv.so"""
    d = _no_context(case(length, taps, rows, channels, ctx, "noise", mode))
    want_y = long_fwd(tf, d["x"], d["h"], d["pre"], d["post"], d["skip"])
    want_dx, want_dpre = long_dx(tf, d["gy"], d["h"], d["post"], d["x"] if d["pre"] is not None else None, d["pre"], d["skip"])
    want_dh, want_dskip = long_dh(tf, d["x"], d["pre"], d["gy"], d["post"], taps)
    for room in (0, ctx):
        assert _same_bits(run_fwd(tf, d, launch_iters, room=room), want_y), ("y", room)
        dx, dpre = run_dx(tf, d, launch_iters, room=room)
        assert _same_bits(dx, want_dx) and (dpre is None or _same_bits(dpre, want_dpre)), ("dx", room)
        dh, dskip = run_dh(tf, d, room=room)
        assert _same_bits(dh, want_dh) and _same_bits(dskip, want_dskip), ("dh", room)


# ------------------------------------------------------------------------------------------- 5. three chunks out of one buffer

def test_three_chunks_out_of_one_buffer_are_the_whole_sequence_gated_plans(tf):
    """x and pre share ONE buffer [B][C][2][total] through views (sequence stride 2 total for both), gy and post another. Hop-aligned
    chunks with context = halo transform exactly the windows of the whole-sequence plans: y, dx and dpre have their bits."""
    total, taps, rows, channels = 12096, 65, 3, 2
    halo, hop, segs = sr.geometry(total, taps)
    assert (halo, hop, segs) == (64, 4032, 3)
    d = case(total, taps, rows, channels, 0, "noise", gc.EVERY_CASE_MODE, seed=3)
    both = torch.from_numpy(np.stack([d["x"], d["pre"]], axis=2)).to(DEV)             # [B][C][2][total]
    back = torch.from_numpy(np.stack([d["gy"], d["post"]], axis=2)).to(DEV)
    t_x, t_pre, t_gy, t_post = both[:, :, 0], both[:, :, 1], back[:, :, 0], back[:, :, 1]
    t_h, t_skip = torch.from_numpy(np.array(d["h"])).to(DEV), torch.from_numpy(np.array(d["skip"])).to(DEV)
    from tensor_fft_amd import gcconv

    tf.gcconv_cache_clear()
    ys, dxs, dpres = [], [], []
    hist = phist = None
    for k in range(3):
        sl = slice(k * hop, (k + 1) * hop)
        ys.append(tf.gated_chunked_causal_conv(t_x[..., sl], t_h, pre=t_pre[..., sl], post=t_post[..., sl], skip=t_skip, history=hist, pre_history=phist))
        hist, phist = tf.next_history(t_x[..., sl], hist, halo), tf.next_history(t_pre[..., sl], phist, halo)
        assert hist.data_ptr() == t_x.data_ptr() + 2 * ((k + 1) * hop - halo) and phist.data_ptr() == hist.data_ptr() + 2 * total
        fut = (t_gy[..., (k + 1) * hop:(k + 1) * hop + halo], t_post[..., (k + 1) * hop:(k + 1) * hop + halo]) if k < 2 else (None, None)
        dx, dpre = tf.gated_chunked_causal_conv_input_grad(t_gy[..., sl], t_h, x=t_x[..., sl], pre=t_pre[..., sl], post=t_post[..., sl], skip=t_skip,
                                                           future=fut[0], post_future=fut[1])
        dxs.append(dx)
        dpres.append(dpre)
    torch.cuda.synchronize()
    # nothing was copied: every plan's strides are the buffers'
    assert all(k[7:10] == (2 * total, 2 * total, 2 * total) for k in gcconv._fwd_plans) and all(k[7:11] == (2 * total,) * 4 for k in gcconv._dx_plans)
    assert sorted(k[10:] for k in gcconv._fwd_plans) == [(0, 0, 0), (halo, 2 * total, 2 * total)]
    assert sorted(k[11:] for k in gcconv._dx_plans) == [(0, 0, 0), (halo, 2 * total, 2 * total)]
    assert np.array_equal(_bits(both.cpu().numpy()), _bits(np.stack([d["x"], d["pre"]], axis=2)))
    want_y = long_fwd(tf, d["x"], d["h"], d["pre"], d["post"], d["skip"])
    want_dx, want_dpre = long_dx(tf, d["gy"], d["h"], d["post"], d["x"], d["pre"], d["skip"])
    assert _same_bits(torch.cat(ys, -1).cpu().numpy(), want_y), "y of three chunks differs from the whole-sequence gated plan"
    assert _same_bits(torch.cat(dxs, -1).cpu().numpy(), want_dx), "dx of three chunks differs from the whole-sequence gated plan"
    assert _same_bits(torch.cat(dpres, -1).cpu().numpy(), want_dpre), "dpre of three chunks differs from the whole-sequence gated plan"
    tf.gcconv_cache_clear()


# ------------------------------------------------------------------------------------------- 6. the contract

def test_a_gate_context_goes_with_its_sequence_context_and_its_gate(tf):
    length, taps, rows, channels, hn = 4104, 7, 2, 2, 8
    n = rows * channels * length
    z = torch.zeros(4 * n, dtype=torch.float16, device=DEV)
    a, b, c, y = (z[i * n:].data_ptr() for i in range(4))
    stream = torch.cuda.current_stream().cuda_stream
    h = torch.zeros(channels * taps, dtype=torch.float16, device=DEV)
    dh = torch.zeros(channels * taps, dtype=torch.float32, device=DEV)
    for pre_gate, post_gate in ((True, True), (False, False)):
        fwd = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, pre_gate=pre_gate, post_gate=post_gate, history=hn)
        grad = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre_gate, post_gate=post_gate, history=hn, future=hn)
        fwd.set_taps(h)
        grad.set_taps(h)
        pre, post, x = (b if pre_gate else None), (c if post_gate else None), (a if pre_gate else None)
        if pre_gate:
            # a gate's context absent with its sequence's context present, and present without it
            with pytest.raises(tf.TfftError, match="pre_hist is NULL but hist is not"):
                fwd.exec_ptr(a, y, pre, post, a, None, stream)
            with pytest.raises(tf.TfftError, match="pre_hist must be NULL when hist is NULL"):
                fwd.exec_ptr(a, y, pre, post, None, b, stream)
            with pytest.raises(tf.TfftError, match="post_future is NULL but gy_future is not"):
                grad.input_grad_ptr(a, y, post, x, pre, None, a, None, stream)
            with pytest.raises(tf.TfftError, match="post_future must be NULL when gy_future is NULL"):
                grad.input_grad_ptr(a, y, post, x, pre, None, None, c, stream)
            with pytest.raises(tf.TfftError, match="pre_hist is NULL but x_hist is not"):
                grad.tap_grad_ptr(a, a, dh.data_ptr(), pre, post, None, a, None, stream)
            with pytest.raises(tf.TfftError, match="pre_hist must be NULL when x_hist is NULL"):
                grad.tap_grad_ptr(a, a, dh.data_ptr(), pre, post, None, None, b, stream)
            with pytest.raises(tf.TfftError, match="16-byte aligned"):
                fwd.exec_ptr(a, y, pre, post, a, b + 2, stream)
        else:
            # a gate's context on a plan without that gate
            with pytest.raises(tf.TfftError, match="pre_hist must be NULL: the plan has no pre gate"):
                fwd.exec_ptr(a, y, None, None, a, b, stream)
            with pytest.raises(tf.TfftError, match="post_future must be NULL: the plan has no post gate"):
                grad.input_grad_ptr(a, y, None, None, None, None, a, c, stream)
            with pytest.raises(tf.TfftError, match="pre_hist must be NULL: the plan has no pre gate"):
                grad.tap_grad_ptr(a, a, dh.data_ptr(), None, None, None, a, b, stream)
        fwd.close()
        grad.close()
    # a context on a plan created without room for one
    fwd = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, pre_gate=True)
    fwd.set_taps(h)
    with pytest.raises(tf.TfftError, match="hist must be NULL: the plan was created with history = 0"):
        fwd.exec_ptr(a, y, b, None, a, b, stream)
    fwd.close()
    torch.cuda.synchronize()
    assert not z.cpu().numpy().any() and not dh.cpu().numpy().any(), "a refused call launched something"


def test_outputs_overlapping_inputs_gates_or_contexts_are_refused_and_nothing_is_launched(tf):
    length, taps, rows, channels, hn = 4104, 7, 2, 2, 8
    d = case(length, taps, rows, channels, hn, "noise", gc.EVERY_CASE_MODE, seed=8)
    seqs, stride = rows * channels, length + 64
    span = seqs * stride
    # one buffer of five spans of sequences `stride` apart, each with 64 halves in front of it: x, pre, post, gy, and a free one
    buf = torch.zeros(5 * span, dtype=torch.float16, device=DEV)
    for i, k in enumerate(("x", "pre", "post", "gy")):
        v = buf[i * span:(i + 1) * span].view(seqs, stride)
        v[:, 64:] = _dev(d[k]).view(seqs, length)
        v[:, :64] = 0.5
    before = buf.cpu().numpy().view(np.uint16).copy()
    stream = torch.cuda.current_stream().cuda_stream
    x, pre, post, gy, free = (buf.data_ptr() + 2 * (i * span + 64) for i in range(5))
    hist, phist, fut, pfut = x - 2 * hn, pre - 2 * hn, gy + 2 * length, post + 2 * length      # the zero-copy call: views in front and behind
    kw = dict(pre_gate=True, post_gate=True)
    fwd = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, in_seq_stride=stride, out_seq_stride=stride, pre_seq_stride=stride,
                                      post_seq_stride=stride, history=hn, hist_seq_stride=stride, pre_hist_seq_stride=stride, **kw)
    grad = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=stride, pre_seq_stride=stride, gy_seq_stride=stride,
                                           post_seq_stride=stride, dx_seq_stride=stride, dpre_seq_stride=stride, history=hn, hist_seq_stride=stride,
                                           pre_hist_seq_stride=stride, future=hn, fut_seq_stride=stride, post_fut_seq_stride=stride, **kw)
    fwd.set_taps(_dev(d["h"]), _dev(d["skip"]))
    grad.set_taps(_dev(d["h"]), _dev(d["skip"]))
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    dskip = torch.zeros((channels,), dtype=torch.float32, device=DEV)
    # the forward output on the input (exact, shifted by a chunk, on its last chunk), on either gate, on either history (the 8 halves
    # in front of the sequences: an output that ENDS there)
    for dst, msg in ((x, "input and output overlap"), (x + 16, "input and output overlap"), (x + 2 * (length - 8), "input and output overlap"),
                     (pre, "the pre gate and the output overlap"), (post + 16, "the post gate and the output overlap")):
        with pytest.raises(tf.TfftError, match=msg):
            fwd.exec_ptr(x, dst, pre, post, hist, phist, stream)
    # dx and dpre on every input and gate of the input gradient
    for dst, msg in ((gy, "gy and "), (post, "post and "), (x + 16, "x and "), (pre, "pre and ")):
        with pytest.raises(tf.TfftError, match=msg + "dx overlap"):
            grad.input_grad_ptr(gy, dst, post, x, pre, free, fut, pfut, stream)
        with pytest.raises(tf.TfftError, match=msg + "dpre overlap"):
            grad.input_grad_ptr(gy, free, post, x, pre, dst, fut, pfut, stream)
    # An output on a context alone, element-exact on the context's own length and stride: contexts of 8 halves, `stride` apart, in a
    # buffer of their own; an output whose last (or first) chunk is the context is refused
    scr = torch.zeros(span + 2 * length, dtype=torch.float16, device=DEV)
    ctx = scr.data_ptr() + 2 * length
    for dst in (ctx - 2 * (length - 8), ctx):
        with pytest.raises(tf.TfftError, match="hist and output overlap"):
            fwd.exec_ptr(x, dst, pre, post, ctx, phist, stream)
        with pytest.raises(tf.TfftError, match="pre_hist and output overlap"):
            fwd.exec_ptr(x, dst, pre, post, hist, ctx, stream)
        with pytest.raises(tf.TfftError, match="gy_future and dx overlap"):
            grad.input_grad_ptr(gy, dst, post, x, pre, free, ctx, pfut, stream)
        with pytest.raises(tf.TfftError, match="post_future and dpre overlap"):
            grad.input_grad_ptr(gy, free, post, x, pre, dst, fut, ctx, stream)
    torch.cuda.synchronize()
    assert not scr.cpu().numpy().any()
    with pytest.raises(tf.TfftError, match="dx and dpre overlap"):
        grad.input_grad_ptr(gy, free, post, x, pre, free + 16, fut, pfut, stream)
    # the tap gradient and the skip gradient on x, on the pre gate's history, on gy; and on each other
    for bad in (x, phist, gy + 2 * (span - 64) - 4 * channels * taps):
        with pytest.raises(tf.TfftError, match="the tap gradient overlaps"):
            grad.tap_grad_ptr(x, gy, bad, pre, post, dskip.data_ptr(), hist, phist, stream)
        with pytest.raises(tf.TfftError, match="the skip gradient overlaps"):
            grad.tap_grad_ptr(x, gy, dh.data_ptr(), pre, post, bad, hist, phist, stream)
    with pytest.raises(tf.TfftError, match="the tap gradient and the skip gradient overlap"):
        grad.tap_grad_ptr(x, gy, dh.data_ptr(), pre, post, dh.data_ptr(), hist, phist, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint16), before) and not dh.cpu().numpy().any() and not dskip.cpu().numpy().any()
    # input-side aliasing is accepted: hist = x - Hn and pre_hist = pre - Hn with the buffers' own strides, x as its own gate and context
    half = np.full((rows, channels, hn), 0.5, np.float16)
    fwd.exec_ptr(x, free, pre, post, hist, phist, stream)
    torch.cuda.synchronize()
    got = buf[4 * span:].view(seqs, stride)[:, 64:].cpu().numpy().reshape(d["x"].shape)
    assert _same_bits(got, run_fwd(tf, dict(d, hist=half, pre_hist=half)))
    fwd.exec_ptr(x, free, x, x, hist, hist, stream)
    grad.input_grad_ptr(gy, free, gy, x, x, None, fut, fut, stream)
    grad.tap_grad_ptr(x, x, dh.data_ptr(), x, x, dskip.data_ptr(), hist, hist, stream)
    torch.cuda.synchronize()
    assert np.array_equal(buf[:4 * span].cpu().numpy().view(np.uint16), before[:4 * span])
    assert np.isfinite(dh.cpu().numpy()).all() and np.array_equal(_bits(dskip.cpu().numpy()), _bits(dh.cpu().numpy()[:, 0].copy()))
    fwd.close()
    grad.close()


def test_exec_needs_taps(tf):
    length, taps, rows, channels = 4104, 7, 2, 2
    fwd = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, history=8)
    grad = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, future=8)
    d_x = torch.zeros(rows * channels * length, dtype=torch.float16, device=DEV)
    d_y = torch.zeros_like(d_x)
    with pytest.raises(tf.TfftError, match="set_taps"):
        fwd.exec(d_x, d_y)
    with pytest.raises(tf.TfftError, match="set_taps"):
        fwd.spectrum()
    with pytest.raises(tf.TfftError, match="set_taps"):
        grad.input_grad(d_x, d_y)
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    grad.tap_grad(d_x, d_x, dh)                                                   # the tap gradient needs no taps
    torch.cuda.synchronize()
    assert not dh.cpu().numpy().any()
    fwd.close()
    grad.close()


def test_launch_iters_never_changes_results(tf):
    d = case(6152, 130, 5, 3, 136, "noise", gc.EVERY_CASE_MODE, seed=4)
    y, (dx, dpre) = run_fwd(tf, d, 0), run_dx(tf, d, 0)
    for iters in (1, 2, 5, 65535):
        assert _same_bits(run_fwd(tf, d, iters), y), iters
        got_dx, got_dpre = run_dx(tf, d, iters)
        assert _same_bits(got_dx, dx) and _same_bits(got_dpre, dpre), iters


def test_executions_with_contexts_under_stream_capture(tf):
    length, taps, rows, channels, ctx = 8064, 65, 2, 3, 64
    d = case(length, taps, rows, channels, ctx, "noise", gc.EVERY_CASE_MODE, seed=6)
    want_y, (want_dx, want_dpre), (want_dh, want_dskip) = run_fwd(tf, d), run_dx(tf, d), run_dh(tf, d)
    kw = dict(pre_gate=True, post_gate=True)
    fwd = tf.TfftGatedChunkedConvPlan(rows, channels, length, taps, 0, history=ctx, **kw)
    grad = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, history=ctx, future=ctx, **kw)
    t = {k: _dev(v) for k, v in d.items()}
    fwd.set_taps(t["h"], t["skip"])
    grad.set_taps(t["h"], t["skip"])
    grad.prepare()                                                                # a prepared plan only launches
    d_y, d_dx, d_dpre = (torch.zeros_like(t["x"]) for _ in range(3))
    dh = torch.zeros((channels, taps), dtype=torch.float32, device=DEV)
    dskip = torch.zeros((channels,), dtype=torch.float32, device=DEV)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fwd.exec(t["x"], d_y, pre=t["pre"], post=t["post"], hist=t["hist"], pre_hist=t["pre_hist"])
            grad.input_grad(t["gy"], d_dx, post=t["post"], x=t["x"], pre=t["pre"], dpre=d_dpre, future=t["fut"], post_future=t["post_fut"])
            grad.tap_grad(t["x"], t["gy"], dh, pre=t["pre"], post=t["post"], dskip=dskip, history=t["hist"], pre_history=t["pre_hist"])
    for _ in range(2):
        for o in (d_y, d_dx, d_dpre, dh, dskip):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((d_y, want_y), (d_dx, want_dx), (d_dpre, want_dpre), (dh, want_dh), (dskip, want_dskip)):
            assert _same_bits(got.cpu().numpy().reshape(want.shape), want)
    fwd.close()
    grad.close()


def test_every_instantiation_is_launched_and_named(tf):
    """the four gate combinations on one small case with a context: each plan names its instantiation, and each result is the shipped
    gated plan's on the concatenated sequences (so the instantiation that ran is the one that was named)"""
    length, taps, rows, channels, ctx = 4104, 7, 3, 3, 8
    hop = sr.geometry(length, taps)[1]
    named = set()
    for mode in ("pre", "post", "pre+post", "skip"):
        d = case(length, taps, rows, channels, ctx, "noise", mode)
        has = (d["pre"] is not None, d["post"] is not None)
        named.update(fwd_kernels(*has) + grad_kernels(*has))
        cx, cpre, cpost = gc.forward_concat(d, taps)
        assert _same_bits(run_fwd(tf, d), long_fwd(tf, cx, d["h"], cpre, cpost, d["skip"])[:, :, hop:]), mode
        cgy, cpost, cx, cpre = gc.input_grad_concat(d)
        dx, dpre = run_dx(tf, d)
        want_dx, want_dpre = long_dx(tf, cgy, d["h"], cpost, cx, cpre, d["skip"])
        assert _same_bits(dx, want_dx[:, :, :length]) and (dpre is None or _same_bits(dpre, want_dpre[:, :, :length])), mode
        cx, cpre, cgy, cpost = gc.tap_grad_concat(d, taps)
        assert _same_bits(run_dh(tf, d, partials=1)[0], long_dh(tf, cx, cpre, cgy, cpost, taps, partials=1)[0]), mode
    assert len(named) == 13, sorted(named)


# ------------------------------------------------------------------------------------------- 7. autograd

def _within(got, want, tol, what):
    err = np.abs(np.asarray(got).astype(np.float64) - want)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{what}: worst {worst:.3f} of its tolerance")
    assert (err <= tol).all(), f"{what}: {worst:.3f} of its tolerance"


def test_autograd_over_two_chunks(tf):
    """Two chunks of (4104, 7, 3, 3) with both gates and a skip; the second chunk's histories are views of the first chunk's x and pre.
    The reference is torch.autograd through an fp64 conv1d of the WHOLE operator at length 2 L (tests/gbconv_ref.py). What autograd
    adds: x1.grad = dx of chunk 1 (no future) + the history's gradient on its last Hn samples, pre1.grad likewise, h.grad =
    fp16(dh1) + fp16(dh2), skip.grad likewise. The tolerances are those tests/gbconv_ref.py derives (du_input_rounding,
    dh_input_rounding, K_SCONV + 1), each on the windows of the plan that computed the term, summed where autograd sums, plus half a
    binary16 ulp of the result for every rounding autograd or a cast adds."""
    length, taps, rows, channels = 4104, 7, 3, 3
    halo, hop, segs = sr.geometry(length, taps)
    k = gc.K_SCONV + 1.0
    w = gc.case_data(2 * length, taps, rows, channels, 0, "noise", 7, gc.EVERY_CASE_MODE)
    lo, hi = slice(0, length), slice(length, 2 * length)
    tf.gcconv_cache_clear()
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(True)    # noqa: E731
    t = {f"{n}{i + 1}": leaf(w[n][:, :, s]) for n in ("x", "pre", "post") for i, s in enumerate((lo, hi))}
    t_h, t_skip = leaf(w["h"]), leaf(w["skip"])
    y1 = tf.differentiable_gated_chunked_causal_conv(t["x1"], t_h, pre=t["pre1"], post=t["post1"], skip=t_skip)
    hist, phist = tf.next_history(t["x1"], None, halo), tf.next_history(t["pre1"], None, halo)
    assert hist.data_ptr() == t["x1"].data_ptr() + 2 * (length - halo) and phist.data_ptr() == t["pre1"].data_ptr() + 2 * (length - halo)
    y2 = tf.differentiable_gated_chunked_causal_conv(t["x2"], t_h, pre=t["pre2"], post=t["post2"], skip=t_skip, history=hist, pre_history=phist)
    y = torch.cat([y1, y2], -1)
    from tensor_fft_amd import gcconv

    assert len(gcconv._fwd_plans) == 2 and not gcconv._dx_plans and not gcconv._dh_plans
    y.backward(torch.from_numpy(w["gy"]).to(DEV))
    torch.cuda.synchronize()
    grads = {n: v.grad.cpu().numpy() for n, v in dict(t, h=t_h, skip=t_skip).items()}
    assert all(g.dtype == np.float16 for g in grads.values())
    want = gb.autograd_reference(w["x"], w["h"], w["pre"], w["post"], w["skip"], w["gy"])
    # the two chunks as the plans saw them
    c1 = {n: (None if w[n] is None or n in ("h", "skip") else w[n][:, :, lo]) for n in w}
    c2 = {n: (None if w[n] is None or n in ("h", "skip") else w[n][:, :, hi]) for n in w}
    for c in (c1, c2):
        c.update(h=w["h"], skip=w["skip"])
    c2.update(hist=w["x"][:, :, length - halo:length], pre_hist=w["pre"][:, :, length - halo:length])
    # the forward pass: chunk 1 is the shipped gated plan, chunk 2 within K_SCONV + 1 of the true operator
    got_y = y.detach().cpu().numpy()
    assert _same_bits(got_y[:, :, lo], long_fwd(tf, c1["x"], w["h"], c1["pre"], c1["post"], w["skip"]))
    peak = sr.window_peak(gc.reference_true(c2))
    _within(got_y[:, :, hi], gc.y_direct(dict(c2, x=gb.gated(c2["x"], c2["pre"]), hist=gb.gated(c2["hist"], c2["pre_hist"]), pre=None, pre_hist=None)),
            gs.post_gate_tolerance(got_y[:, :, hi], c2["post"], k, peak, rows, channels, length, taps), "y2")
    # ---- x.grad and pre.grad. Chunk 2 and the front of chunk 1 are one plan's dx / dpre: gbconv_ref.dx_tolerance on that chunk's windows
    before = {}
    for name, c, s in (("1", c1, lo), ("2", c2, hi)):
        du_peak = sr.window_peak(gc.du_windows_true(c))
        before[name] = k * gb.per_sample(eb.ulp16(du_peak), rows, channels, length, taps) + gc.du_input_rounding(c)
    for which, gate in (("x", "pre"), ("pre", "x")):
        _within(grads[which + "2"], want["d" + which][:, :, hi], gb.gated_tolerance(grads[which + "2"], c2[gate], before["2"]), which + "2.grad")
    # the histories' gradients: the input gradient at length Hn on a zero gy whose future is the start of chunk 2's gy and post
    n = min(length, gc.carry_min(taps))
    ch = dict(gy=np.zeros((rows, channels, halo), np.float16), post=np.ones((rows, channels, halo), np.float16), fut=c2["gy"][:, :, :n],
              post_fut=c2["post"][:, :, :n], h=w["h"], skip=w["skip"], x=c2["hist"], pre=c2["pre_hist"], hist=None, pre_hist=None)
    h_before = k * gb.per_sample(eb.ulp16(sr.window_peak(gc.du_windows_true(ch))), rows, channels, halo, taps) + gc.du_input_rounding(ch)
    true_h = gc.input_grad_direct(ch)
    true_1 = gc.input_grad_direct(c1)
    tail = slice(length - halo, length)
    for i, (which, gate) in enumerate((("x", "pre"), ("pre", "x"))):
        got, ref = grads[which + "1"], want["d" + which][:, :, lo]
        assert np.abs(true_1[i][:, :, tail] + true_h[i] - ref[:, :, tail]).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        tol = gb.gated_tolerance(got, c1[gate], before["1"])                     # in front of the tail: dx (dpre) of chunk 1 alone
        # on the tail autograd adds two binary16 values: each term's own bound (its rounding taken at the true value plus the bound in
        # front of it), and half an ulp of the sum
        g1, gh = np.abs(c1[gate].astype(np.float64))[:, :, tail] * before["1"][:, :, tail], np.abs(ch[gate].astype(np.float64)) * h_before
        t1 = g1 + 0.5 * eb.ulp16(np.abs(true_1[i][:, :, tail]) + g1)
        th = gh + 0.5 * eb.ulp16(np.abs(true_h[i]) + gh)
        tol[:, :, tail] = t1 + th + 0.5 * eb.ulp16(np.abs(ref[:, :, tail]) + t1 + th)
        _within(got, ref, tol, which + "1.grad")
    # ---- post.grad: the forward plan with gy as its post gate, chunk by chunk
    _within(grads["post1"], want["dpost"][:, :, lo], gb.dpost_tolerance(grads["post1"], c1["x"], w["h"], c1["pre"], w["skip"], c1["gy"]), "post1.grad")
    _within(grads["post2"], want["dpost"][:, :, hi], gs.post_gate_tolerance(grads["post2"], c2["gy"], k, peak, rows, channels, length, taps), "post2.grad")
    # ---- h.grad and skip.grad: dh1 + dh2, each within its dh_bound and input rounding, cast to binary16, added by autograd
    b1 = br.dh_bound(gc.dh_items(c1, taps), channels)[:, None] + gc.dh_input_rounding(c1, taps)
    b2 = br.dh_bound(gc.dh_items(c2, taps), channels)[:, None] + gc.dh_input_rounding(c2, taps)
    d1, d2 = gc.dh_direct(c1, taps), gc.dh_direct(c2, taps)
    assert np.abs(d1 + d2 - want["dh"]).max() <= 1e-12 * max(1.0, np.abs(want["dh"]).max())
    tol_dh = b1 + b2 + 0.5 * (eb.ulp16(np.abs(d1) + b1) + eb.ulp16(np.abs(d2) + b2))
    tol_dh = tol_dh + 0.5 * eb.ulp16(np.abs(want["dh"]) + tol_dh)
    _within(grads["h"], want["dh"], tol_dh, "h.grad")
    _within(grads["skip"], want["dskip"], tol_dh[:, 0], "skip.grad")
    tf.gcconv_cache_clear()


def test_each_gradient_runs_only_when_asked(tf):
    from tensor_fft_amd import gcconv

    length, taps, rows, channels = 4104, 7, 3, 3
    halo = sr.geometry(length, taps)[0]
    d = case(length, taps, rows, channels, halo, "noise", gc.EVERY_CASE_MODE, seed=7)
    names = ("x", "h", "pre", "post", "skip", "hist", "pre_hist")
    t_gy = torch.from_numpy(np.array(d["gy"])).to(DEV)
    for need in [(n,) for n in names] + [names]:
        tf.gcconv_cache_clear()
        a = {n: torch.from_numpy(d[n].copy()).to(DEV).requires_grad_(n in need) for n in names}
        y = tf.differentiable_gated_chunked_causal_conv(a["x"], a["h"], pre=a["pre"], post=a["post"], skip=a["skip"], history=a["hist"],
                                                        pre_history=a["pre_hist"])
        assert len(gcconv._fwd_plans) == 1
        y.backward(t_gy)
        torch.cuda.synchronize()
        assert [n for n in names if a[n].grad is not None] == list(need), need
        # the input gradient's cache holds the plan of dx / dpre (length L) and the one of the histories (length Hn); dpost is one more
        # forward plan (gy as the post gate: the same key, so no new plan)
        want_dx = int(bool({"x", "pre"} & set(need))) + int(bool({"hist", "pre_hist"} & set(need)))
        assert (len(gcconv._dx_plans), len(gcconv._dh_plans), len(gcconv._fwd_plans)) == (want_dx, int(bool({"h", "skip"} & set(need))), 1), need
    # the histories' gradients against their definition: pre_history (.) du_h and history (.) du_h
    n = min(length, gc.carry_min(taps))
    ch = dict(gy=np.zeros((rows, channels, halo), np.float16), post=np.ones((rows, channels, halo), np.float16), fut=d["gy"][:, :, :n],
              post_fut=d["post"][:, :, :n], h=d["h"], skip=d["skip"], x=d["hist"], pre=d["pre_hist"], hist=None, pre_hist=None)
    before = ((gc.K_SCONV + 1.0) * gb.per_sample(eb.ulp16(sr.window_peak(gc.du_windows_true(ch))), rows, channels, halo, taps)
              + gc.du_input_rounding(ch))
    true_h = gc.input_grad_direct(ch)
    _within(a["hist"].grad.cpu().numpy(), true_h[0], gb.gated_tolerance(a["hist"].grad.cpu().numpy(), d["pre_hist"], before), "history.grad")
    _within(a["pre_hist"].grad.cpu().numpy(), true_h[1], gb.gated_tolerance(a["pre_hist"].grad.cpu().numpy(), d["hist"], before), "pre_history.grad")
    tf.gcconv_cache_clear()


def test_strided_views_are_not_copied(tf):
    """a chunk of a longer buffer, its gates and their contexts go to the plans as they are: every stride of the plan is the
    buffer's, and the tap gradient is the bits of the plan run by hand on dense copies"""
    from tensor_fft_amd import gcconv

    total, taps, rows, channels = 8136, 7, 3, 3
    length, ctx = 4104, 8
    w = gc.case_data(total, taps, rows, channels, 0, "noise", 5, gc.EVERY_CASE_MODE)
    t = {n: torch.from_numpy(w[n]).to(DEV) for n in ("x", "pre", "post", "gy", "h", "skip")}
    sl, hs = slice(total - length, total), slice(total - length - ctx, total - length)
    tf.gcconv_cache_clear()
    dh, dskip = tf.gated_chunked_causal_conv_tap_grad(t["x"][..., sl], t["gy"][..., sl], taps, pre=t["pre"][..., sl], post=t["post"][..., sl],
                                                      history=t["x"][..., hs], pre_history=t["pre"][..., hs])
    torch.cuda.synchronize()
    (key,) = gcconv._dh_plans
    assert key[7:] == (total, total, total, total, ctx, total, total), key
    d = {n: (w[n][:, :, sl] if n in ("x", "pre", "post", "gy") else w[n]) for n in ("x", "pre", "post", "gy", "h", "skip")}
    d.update(hist=w["x"][:, :, hs], pre_hist=w["pre"][:, :, hs], fut=None, post_fut=None)
    want_dh, want_dskip = run_dh(tf, d)
    assert _same_bits(dh.cpu().numpy(), want_dh) and _same_bits(dskip.cpu().numpy(), want_dskip)
    tf.gcconv_cache_clear()


# ------------------------------------------------------------------------------------------- 9. the example

def test_example_gated_chunked_conv_exits_0(tf):
    exe = os.path.join(ROOT, "examples", "example_gated_chunked_conv")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout

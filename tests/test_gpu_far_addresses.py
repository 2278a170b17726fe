"""Every plan that takes a stride, with its sequences placed beyond 2, 4 and 8 GiB of one allocation (tests/far_layout.py).

The headers promise 64-bit strides; the other suites run with strides of L + 8 and L + 24, where a `row * stride` formed in 32
bits, or a stride narrowed on its way from Python through ctypes into an options struct, gives the right answer. Here the strides
are 2^31 + 8 / 2^31 + 24 halves (layout `wide`, 3 rows x 1 channel) and 2^30 + 8 / 2^30 + 24 (`channels`, 2 rows x 2 channels), so
blocks start in (2^31, 2^32), in (2^32, 2^33) and beyond 2^33 bytes, and a start index in halves exceeds 2^32.

Each case runs the plan twice through the same code (Run below): in the far arenas, and with the plan's default dense strides in
two small arenas. It asserts

  a. the far result is the dense result in every bit (a plan's result does not depend on its strides),
  b. the far result meets the family's own yardsticks: the family's GPU test module checks it, with its `run_*` function replaced
     by the far run (pytest's monkeypatch), so the references, constants and comparisons are the family's own and nothing is
     restated here; the core plans are held to the fp64 oracle under the constants of tests/test_gpu_kernel_matrix.py,
  c. every half of the output arena outside the blocks the plan owns still holds the NaN sentinel: a store through a truncated
     offset lands in a gap or in another sequence,
  d. the input arena comes back bit for bit, its gaps NaN: a load through a truncated offset poisons (a) or reads another
     sequence's data.

Inputs, gates and contexts of one execution share the input arena at small distinct bases with equal strides; outputs have the
output arena. The shapes are the smallest at which a kernel's indexing is non-trivial: for the overlap-save families L = 4104,
K = 7 (halo 64, a second segment of 9 chunks) and L = 4096, K = 2049 (halo = hop). No tolerance of this file's own.

A test holds at most two far arenas (28 GiB at the most: a frame-strided side of 6 frames and a signal side of 3 rows at stride
2^31) and skips only where the device has less than that plus 4 GiB free. Filling and scanning an arena takes milliseconds."""
import numpy as np
import pytest

import bconv_ref as br
import elementwise_bound as eb
import far_layout as fl
import gcconv_ref as gc
import gconv_ref as gr
import gsconv_ref as gs
import istft_ref as ir
import istftn_ref as inr
import lconv_ref as lr
import sconv_ref as sr
import stft_ref as st
import stftn_ref as sn

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
LAYOUTS = list(fl.LAYOUTS)
SLOT = 1 << 14                  # halves between the far bases of the tensors that share an arena (64 of them fit fl.ROOM)
DENSE = 1 << 21                 # halves of a dense arena
LONG_SHAPES = [(4104, 7), (4096, 2049)]      # (L, K) of the overlap-save families
SIX = fl.FRAME_ROWS * fl.FRAMES_PER_ROW


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


@pytest.fixture(scope="module")
def pool():
    p = fl.Pool(torch, DEV)
    yield p
    p.release()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a).reshape(-1)).to(DEV)


def _half(t):
    return t.view(torch.float16)


class Run:
    """One execution's tensors in a pair of arenas: far (the layout's strides, bases in slots of SLOT halves) or dense (the plan's
    default strides, tensors back to back). The family code below is written once against this and runs in both."""

    def __init__(self, arenas, lay, far):
        self.arenas, self.lay, self.far = arenas, lay, far
        self.inputs, self.outputs = [], []
        self.next = {"in": 0, "out": 0}

    def stride(self, side, dense, extra=0):
        """halves between a tensor's runs: the layout's (+ extra) when far, the plan's default when dense"""
        return fl.stride_of(self.lay, side) + extra if self.far else dense

    def opt(self, side, extra=0):
        """what the plan's stride option takes: 0 asks for the default"""
        return fl.stride_of(self.lay, side) + extra if self.far else 0

    def region(self, side, far_halves, dense_halves):
        """the base of a new tensor (or group of tensors laid out by the caller): far_halves per run when far, dense_halves in all"""
        base = self.next[side]
        self.next[side] += -(-far_halves // SLOT) * SLOT if self.far else -(-dense_halves // 8) * 8
        return base

    def put(self, host, base, stride):
        """an input [count][length] at base + q * stride: the flat float16 view a plan is handed"""
        host = np.ascontiguousarray(host)
        block = fl.Block(base, host.shape[0], stride, host.shape[1])
        self.arenas["in"].scatter(block, host)
        self.inputs.append((block, host))
        return _half(self.arenas["in"].view(block))

    def out(self, count, length, base, stride):
        block = fl.Block(base, count, stride, length)
        self.arenas["out"].place(block)
        self.outputs.append(block)
        return _half(self.arenas["out"].view(block))

    def finish(self):
        """(c) and (d); the outputs [count][length] int16, in the order of the out() calls"""
        torch.cuda.synchronize()
        where = "far" if self.far else "dense"
        self.arenas["out"].check_gaps(where + " output arena")
        self.arenas["in"].check_gaps(where + " input arena")
        for block, host in self.inputs:
            self.arenas["in"].check_block(block, host, where + " input arena")
        return [self.arenas["out"].gather(b) for b in self.outputs]


def both(pool, lay, go, counts=None, what=""):
    """go(run) -> tuple of arrays (or None), once far and once dense: asserts (a), returns the far results"""
    counts = counts or {}
    seqs = lay.rows * lay.channels
    sizes = {side: fl.arena_halves(lay, side, max(counts.get(side, 0), seqs)) for side in fl.SIDES}
    short = pool.missing(dict(sizes, din=DENSE, dout=DENSE))
    if short:
        pytest.skip(f"needs {sum(sizes.values()) * 2 >> 30} GiB of HBM and {fl.Pool.HEADROOM >> 30} GiB of headroom: {short >> 20} MiB short")
    arenas = pool.get(dict(sizes, din=DENSE, dout=DENSE))
    far = go(Run({"in": arenas["in"], "out": arenas["out"]}, lay, True))
    dense = go(Run({"in": arenas["din"], "out": arenas["dout"]}, lay, False))
    assert len(far) == len(dense)
    for i, (a, b) in enumerate(zip(far, dense)):
        assert (a is None) == (b is None), (what, i)
        if a is None:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        bits = np.uint16 if a.itemsize == 2 else np.uint32
        bad = np.argwhere(a.view(bits) != b.view(bits))
        assert bad.size == 0, f"{what}: result {i} at far strides differs from the dense execution in {len(bad)} elements, first {bad[:3].tolist()}"
    return far


def _seq_in(r, a):
    """a [B][C][n] input as a tensor of its own: far at the layout's input stride, dense contiguous"""
    a = np.asarray(a)
    seqs, n = a.shape[0] * a.shape[1], a.shape[2]
    return r.put(a.reshape(seqs, n), r.region("in", n, seqs * n), r.stride("in", n))


def _seq_out(r, shape):
    seqs, n = shape[0] * shape[1], shape[2]
    return r.out(seqs, n, r.region("out", n, seqs * n), r.stride("out", n))


def _f32_out(channels, taps, pad=64):
    """dh [C][K] (and dskip [C]) between NaN words"""
    return torch.full((pad + channels * taps + pad + channels + pad,), float("nan"), dtype=torch.float32, device=DEV)


def _f32_read(buf, channels, taps, pad=64):
    """(dh [C][K], dskip [C]) of a buffer of _f32_out; every other word still NaN. A plan without dskip leaves it NaN."""
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo = 2 * pad + channels * taps
    keep = np.ones(host.size, bool)
    keep[pad:pad + channels * taps] = False
    keep[lo:lo + channels] = False
    assert np.isnan(host[keep]).all(), "tap or skip gradient written outside [C][K] / [C]"
    return host[pad:pad + channels * taps].reshape(channels, taps).copy(), host[lo:lo + channels].copy()


def _bcl(runs, shape):
    return fl.to_bcl(runs, shape[0], shape[1])


# ===================================================================================================== the core plans (libtfft.so)

def _complex_case(tf, orc, pool, lay, n, batch=3, inner=1, **kw):
    import test_gpu_kernel_matrix as km

    nf = n * inner
    rng = np.random.default_rng([11, n, batch, inner])
    x = rng.uniform(-1, 1, (batch, 2, nf)).astype(np.float16)
    kernels = []

    def go(r):
        plan = tf.TfftPlan(n, batch, 0, in_batch_stride=r.opt("in"), out_batch_stride=r.opt("out"), preserve_input=True, inner=inner, **kw)
        ws = None
        if plan.workspace_bytes:
            ws = torch.empty(plan.workspace_bytes // 2, dtype=torch.float16, device=DEV)
            plan.set_workspace(ws)
        kernels[:] = plan.kernels
        s_in, s_out = r.stride("in", 2 * nf), r.stride("out", 2 * nf)
        b_in, b_out = r.region("in", 2 * nf, batch * 2 * nf), r.region("out", 2 * nf, batch * 2 * nf)
        re, im = r.put(x[:, 0], b_in, s_in), r.put(x[:, 1], b_in + nf, s_in)
        o_re, o_im = r.out(batch, nf, b_out, s_out), r.out(batch, nf, b_out + nf, s_out)
        plan.exec(re, im, o_re, o_im)
        res = r.finish()
        plan.close()
        return tuple(res)

    what = f"TfftPlan n={n} inner={inner} {kw} {lay.name}"
    g_re, g_im = (a.view(np.float16).astype(np.float64) for a in both(pool, lay, go, {"in": batch, "out": batch}, what))
    if inner == 1:
        e_re, e_im = orc.dft64(x[:, 0], x[:, 1])
        ref = e_re + 1j * e_im
    else:
        xc = (x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)).reshape(batch, n, inner)
        ref = (np.fft.fft(xc, axis=1) / n).reshape(batch, nf)
    eb.check(g_re, g_im, ref.real, ref.imag, km.k_of(kernels, {"kind": "c"}), what=what)
    return kernels


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096, 8192, 1 << 16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_complex_plans(tf, orc, pool, layout, n):
    """the default plan of each length at batch 3: the one-pass kernels up to 4096, the latency pair at 8192, a two-pass chain at 2^16"""
    kernels = _complex_case(tf, orc, pool, fl.LAYOUTS[layout], n)
    print(f"TfftPlan n={n} batch=3 {layout}: {kernels}")
    assert len(kernels) >= 2 if n == 1 << 16 else len(kernels) <= 2, kernels


@pytest.mark.parametrize("layout", LAYOUTS)
def test_complex_plan_8192_in_one_pass(tf, orc, pool, layout):
    """n = 8192 without the latency kernels: the plan a large batch gets (k4096r)"""
    from tensor_fft_amd import capi

    kernels = _complex_case(tf, orc, pool, fl.LAYOUTS[layout], 8192, variant=capi.VARIANT_NO_LATENCY_KERNEL)
    print(f"TfftPlan n=8192 batch=3 NO_LATENCY_KERNEL {layout}: {kernels}")
    assert not any("collat" in k for k in kernels), kernels


@pytest.mark.parametrize("layout", LAYOUTS)
def test_complex_plan_stockham_chain(tf, orc, pool, layout):
    from tensor_fft_amd import capi

    kernels = _complex_case(tf, orc, pool, fl.LAYOUTS[layout], 1024, variant=capi.VARIANT_AUTOSORT_ONLY)
    assert all(k.startswith("stockham::") for k in kernels), kernels


@pytest.mark.parametrize("layout", LAYOUTS)
def test_complex_plan_on_a_strided_axis(tf, orc, pool, layout):
    kernels = _complex_case(tf, orc, pool, fl.LAYOUTS[layout], 256, inner=16)
    assert any(k.startswith("colfft::") for k in kernels), kernels


@pytest.mark.parametrize("n,two_pass", [(4096, False), (8192, True)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_real_plans(tf, pool, layout, n, two_pass):
    """R2C, then C2R of half spectra of binary16 size (tests/test_gpu_kernel_matrix.py, run_real): K_REAL, pair by pair"""
    lay, batch = fl.LAYOUTS[layout], 3
    h = n // 2 + 1
    rng = np.random.default_rng([12, n, batch])
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float16)
    spec = np.fft.rfft(x.astype(np.float64), axis=1) / np.sqrt(n)
    s_re, s_im = spec.real.astype(np.float16), spec.imag.astype(np.float16)

    def r2c(r):
        plan = tf.TfftRealPlan(n, batch, 0, in_batch_stride=r.opt("in"), out_batch_stride=r.opt("out"), two_pass=two_pass)
        pitch = plan.pitch
        vx = r.put(x, r.region("in", n, batch * n), r.stride("in", n))
        b = r.region("out", 2 * pitch, batch * 2 * pitch)
        o_re, o_im = r.out(batch, h, b, r.stride("out", 2 * pitch)), r.out(batch, h, b + pitch, r.stride("out", 2 * pitch))
        plan.r2c(vx, o_re, o_im)
        res = r.finish()
        plan.close()
        return tuple(res)

    def c2r(r):
        # in_batch_stride is the signals' and out_batch_stride the spectra's in both directions: here the spectra are the input, in
        # the input arena, so the two options change sides
        plan = tf.TfftRealPlan(n, batch, 0, in_batch_stride=r.opt("out"), out_batch_stride=r.opt("in"), two_pass=two_pass)
        pitch = plan.pitch
        b = r.region("in", 2 * pitch, batch * 2 * pitch)
        i_re, i_im = r.put(s_re, b, r.stride("in", 2 * pitch)), r.put(s_im, b + pitch, r.stride("in", 2 * pitch))
        vy = r.out(batch, n, r.region("out", n, batch * n), r.stride("out", n))
        plan.c2r(i_re, i_im, vy)
        res = r.finish()
        plan.close()
        return tuple(res)

    what = f"TfftRealPlan n={n} two_pass={two_pass} {layout}"
    g_re, g_im = (a.view(np.float16).astype(np.float64) for a in both(pool, lay, r2c, {"in": batch, "out": batch}, what + " r2c"))
    ref = np.fft.rfft(x.astype(np.float64), axis=1) / n
    eb.check(g_re, g_im, ref.real, ref.imag, eb.K_REAL, pairs=True, what=what + " r2c")
    got = both(pool, lay, c2r, {"in": batch, "out": batch}, what + " c2r")[0].view(np.float16).astype(np.float64)
    want = np.fft.irfft(s_re.astype(np.float64) + 1j * s_im.astype(np.float64), n, axis=1)
    eb.check(got, np.zeros_like(got), want, np.zeros_like(want), eb.K_REAL, pairs=True, what=what + " c2r")


# ======================================================================================================= libtfft_conv.so

@pytest.mark.parametrize("n,composed", [(4096, False), (256, True)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_conv(tf, pool, layout, n, composed, monkeypatch):
    import test_gpu_conv as tc

    lay, batch, filters = fl.LAYOUTS[layout], 3, 2

    def far_run(tf_, n_, batch_, filters_, composed_, x_re, x_im, h_re, h_im, in_place=False, pad=True):
        def go(r):
            plan = tf.TfftConvPlan(n, batch, filters, 0, in_batch_stride=r.opt("in"), out_batch_stride=r.opt("out"), composed=composed)
            plan.set_filter(_dev(h_re), _dev(h_im))
            s_in, s_out = r.stride("in", 2 * n), r.stride("out", 2 * n)
            b_in, b_out = r.region("in", 2 * n, batch * 2 * n), r.region("out", 2 * n, batch * 2 * n)
            re, im = r.put(x_re, b_in, s_in), r.put(x_im, b_in + n, s_in)
            o_re, o_im = r.out(batch, n, b_out, s_out), r.out(batch, n, b_out + n, s_out)
            plan.exec(re, im, o_re, o_im)
            res = r.finish()
            plan.close()
            return tuple(res)

        y_re, y_im = both(pool, lay, go, {"in": batch, "out": batch}, f"conv n={n} composed={composed} {layout}")
        return y_re.view(np.float16), y_im.view(np.float16)

    monkeypatch.setattr(tc, "run_conv", far_run)
    for kind in ("delays", "decay"):
        tc._check_case(tf, n, batch, filters, composed, kind)


# ======================================================================================== libtfft_lconv.so, libtfft_gconv.so

def _far_gated(tf, pool, lay, cls, what, **plan_kw):
    """run_lconv / run_gconv / run_sconv / run_gsconv of the family's test module, at far strides: (y [B][C][L], spectrum)"""

    def far_run(tf_, x, h, p=None, g=None, skip=None, launch_iters=0, gated=True):
        spec = []

        def go(r):
            rows, channels, length = x.shape
            kw = dict(in_seq_stride=r.opt("in"), out_seq_stride=r.opt("out"), launch_iters=launch_iters, **plan_kw)
            if gated:
                kw.update(pre_gate=p is not None, post_gate=g is not None, pre_seq_stride=r.opt("in") if p is not None else 0,
                          post_seq_stride=r.opt("in") if g is not None else 0)
            plan = cls(rows, channels, length, h.shape[1], 0, **kw)
            if gated:
                plan.set_taps(_dev(h), _dev(skip))
            else:
                plan.set_taps(_dev(h))
            spec[:] = [t.cpu().numpy() for t in plan.spectrum()]
            vx = _seq_in(r, x)
            vp = None if p is None else _seq_in(r, p)
            vg = None if g is None else _seq_in(r, g)
            vy = _seq_out(r, x.shape)
            if gated:
                plan.exec(vx, vy, pre=vp, post=vg)
            else:
                plan.exec(vx, vy)
            res = r.finish()
            plan.close()
            return (res[0],) + tuple(spec)

        res = both(pool, lay, go, what=f"{what} {lay.name}")
        return _bcl(res[0], x.shape), tuple(res[1:])

    return far_run


@pytest.mark.parametrize("length,taps", [(520, 7), (2056, 7)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_lconv(tf, pool, layout, length, taps, monkeypatch):
    """fused, and composed at L = 2056: lconv_copy::pack_kernel and crop_kernel around the shipped convolution plan"""
    import test_gpu_lconv as tl

    lay = fl.LAYOUTS[layout]
    far = _far_gated(tf, pool, lay, tf.TfftCausalConvPlan, f"lconv L={length} K={taps}")
    monkeypatch.setattr(tl, "run_lconv", lambda tf_, x, h, launch_iters=0, composed=False: far(tf_, x, h, launch_iters=launch_iters, gated=False))
    plan = tf.TfftCausalConvPlan(lay.rows, lay.channels, length, taps, 0)
    assert (plan.kernels == ["lconv4096::lconv4096_kernel"]) == (length == 520) and ("lconv_copy::pack_kernel" in plan.kernels) == (length == 2056)
    plan.close()
    k = lr.K_LCONV_FUSED if length == 520 else lr.K_LCONV_COMPOSED
    tl.check_case(tf, length, taps, lay.rows, lay.channels, "noise", k)


@pytest.mark.parametrize("length,taps", [(520, 7), (2056, 7)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gconv(tf, pool, layout, length, taps, monkeypatch):
    """both gates and a skip; composed at L = 2056: gate_copy::pack_kernel<true> and crop_kernel<true>"""
    import test_gpu_gconv as tg

    lay = fl.LAYOUTS[layout]
    far = _far_gated(tf, pool, lay, tf.TfftGatedConvPlan, f"gconv L={length} K={taps}")
    monkeypatch.setattr(tg, "run_gconv", lambda tf_, x, h, p=None, g=None, skip=None, launch_iters=0, composed=False: far(tf_, x, h, p, g, skip, launch_iters))
    plan = tf.TfftGatedConvPlan(lay.rows, lay.channels, length, taps, 0, pre_gate=True, post_gate=True)
    assert (plan.kernels == ["gconv4096::gconv4096_kernel<true, true>"]) == (length == 520)
    assert ("gate_copy::pack_kernel<true>" in plan.kernels and "gate_copy::crop_kernel<true>" in plan.kernels) == (length == 2056)
    plan.close()
    k = gr.K_LCONV_FUSED if length == 520 else gr.K_LCONV_COMPOSED
    tg.check_case(tf, length, taps, lay.rows, lay.channels, "noise", "pre+post+skip", k)


# ====================================================================================== libtfft_sconv.so, libtfft_gsconv.so

@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_sconv(tf, pool, layout, length, taps, monkeypatch):
    import test_gpu_sconv as ts

    lay = fl.LAYOUTS[layout]
    far = _far_gated(tf, pool, lay, tf.TfftLongConvPlan, f"sconv L={length} K={taps}")
    monkeypatch.setattr(ts, "run_sconv", lambda tf_, x, h, launch_iters=0: far(tf_, x, h, launch_iters=launch_iters, gated=False))
    ts.check_case(tf, length, taps, lay.rows, lay.channels, "noise")


@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gsconv(tf, pool, layout, length, taps, monkeypatch):
    import test_gpu_gsconv as tg

    lay = fl.LAYOUTS[layout]
    far = _far_gated(tf, pool, lay, tf.TfftGatedLongConvPlan, f"gsconv L={length} K={taps}")
    monkeypatch.setattr(tg, "run_gsconv", lambda tf_, x, h, p=None, g=None, skip=None, launch_iters=0: far(tf_, x, h, p, g, skip, launch_iters))
    tg.check_case(tf, length, taps, lay.rows, lay.channels, "noise", gs.EVERY_CASE_MODE)


# ====================================================================================== libtfft_bconv.so, libtfft_gbconv.so

def _far_bconv_dx(tf, pool, lay):
    def far_run(tf_, g, h, launch_iters=0):
        def go(r):
            rows, channels, length = g.shape
            plan = tf.TfftLongConvGradPlan(rows, channels, length, h.shape[1], 0, g_seq_stride=r.opt("in"), dx_seq_stride=r.opt("out"), launch_iters=launch_iters)
            plan.set_taps(_dev(h))
            spec = [t.cpu().numpy() for t in plan.spectrum()]
            plan.input_grad(_seq_in(r, g), _seq_out(r, g.shape))
            res = r.finish()
            plan.close()
            return (res[0],) + tuple(spec)

        res = both(pool, lay, go, what=f"bconv dgrad {g.shape} K={h.shape[1]} {lay.name}")
        return _bcl(res[0], g.shape), tuple(res[1:])

    return far_run


def _far_bconv_dh(tf, pool, lay, x, g, taps, partials=0):
    def go(r):
        rows, channels, length = x.shape
        plan = tf.TfftLongConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=r.opt("in"), g_seq_stride=r.opt("in"), partials=partials)
        buf = _f32_out(channels, taps)
        plan.tap_grad(_seq_in(r, x), _seq_in(r, g), buf[64:64 + channels * taps])
        r.finish()
        dh, _ = _f32_read(buf, channels, taps)
        plan.close()
        return (dh,)

    return both(pool, lay, go, what=f"bconv wgrad {x.shape} K={taps} {lay.name}")[0]


@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_bconv(tf, pool, layout, length, taps, monkeypatch):
    """the input gradient (far g, far dx) and the tap gradient (far x and g, dense dh)"""
    import test_gpu_bconv as tb

    lay = fl.LAYOUTS[layout]
    monkeypatch.setattr(tb, "run_dgrad", _far_bconv_dx(tf, pool, lay))
    tb.check_dx_case(tf, length, taps, lay.rows, lay.channels, "noise")
    case = (length, taps, lay.rows, lay.channels, 0)
    x, _ = lr.case_data(length, taps, lay.rows, lay.channels, "noise", 1)
    g = br.grad_signal(lay.rows, lay.channels, length, taps, 1)
    dh = _far_bconv_dh(tf, pool, lay, x, g, taps)
    tb.check_dh_against_fp64(case, x, g, dh)
    tb.check_dh_by_composition(tf, case, x, g, dh)


def _far_gbconv_dx(tf, pool, lay):
    def far_run(tf_, gy, h, post=None, x=None, pre=None, skip=None, launch_iters=0, want_dpre=True):
        def go(r):
            rows, channels, length = gy.shape
            s = lambda a: r.opt("in") if a is not None else 0          # noqa: E731
            with_dpre = pre is not None and want_dpre
            plan = tf.TfftGatedLongConvGradPlan(rows, channels, length, h.shape[1], 0, pre_gate=pre is not None, post_gate=post is not None,
                                                x_seq_stride=s(pre), pre_seq_stride=s(pre), gy_seq_stride=r.opt("in"), post_seq_stride=s(post),
                                                dx_seq_stride=r.opt("out"), dpre_seq_stride=r.opt("out") if with_dpre else 0, launch_iters=launch_iters)
            plan.set_taps(_dev(h), _dev(skip))
            spec = [t.cpu().numpy() for t in plan.spectrum()]
            v = {k: (None if a is None else _seq_in(r, a)) for k, a in (("gy", gy), ("post", post), ("x", x if pre is not None else None), ("pre", pre))}
            v_dx = _seq_out(r, gy.shape)
            v_dpre = _seq_out(r, gy.shape) if with_dpre else None
            plan.input_grad(v["gy"], v_dx, post=v["post"], x=v["x"], pre=v["pre"], dpre=v_dpre)
            res = r.finish()
            plan.close()
            return (res[0], res[1] if with_dpre else None) + tuple(spec)

        res = both(pool, lay, go, what=f"gbconv dgrad {gy.shape} K={h.shape[1]} {lay.name}")
        return _bcl(res[0], gy.shape), (None if res[1] is None else _bcl(res[1], gy.shape)), tuple(res[2:])

    return far_run


def _far_gbconv_dh(tf, pool, lay):
    def far_run(tf_, x, pre, gy, post, taps, partials=0, plan=None):
        assert plan is None

        def go(r):
            rows, channels, length = x.shape
            s = lambda a: r.opt("in") if a is not None else 0          # noqa: E731
            p = tf.TfftGatedLongConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre is not None, post_gate=post is not None,
                                             x_seq_stride=r.opt("in"), pre_seq_stride=s(pre), gy_seq_stride=r.opt("in"), post_seq_stride=s(post),
                                             partials=partials)
            v = {k: (None if a is None else _seq_in(r, a)) for k, a in (("x", x), ("pre", pre), ("gy", gy), ("post", post))}
            buf = _f32_out(channels, taps)
            lo = 128 + channels * taps
            p.tap_grad(v["x"], v["gy"], buf[64:64 + channels * taps], pre=v["pre"], post=v["post"], dskip=buf[lo:lo + channels])
            r.finish()
            res = _f32_read(buf, channels, taps)
            p.close()
            return res

        return both(pool, lay, go, what=f"gbconv wgrad {x.shape} K={taps} {lay.name}")

    return far_run


@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gbconv(tf, pool, layout, length, taps, monkeypatch):
    """both gates and a skip: dx and dpre with x, pre, gy and post all far; the tap and skip gradients, dense"""
    import test_gpu_gbconv as tg

    lay = fl.LAYOUTS[layout]
    monkeypatch.setattr(tg, "run_dgrad", _far_gbconv_dx(tf, pool, lay))
    monkeypatch.setattr(tg, "run_wgrad", _far_gbconv_dh(tf, pool, lay))
    tg.check_dx_case(tf, length, taps, lay.rows, lay.channels, "noise", "pre+post+skip")
    tg.check_dh_case(tf, (length, taps, lay.rows, lay.channels, 0, "pre+post"))


# ====================================================================================== libtfft_cconv.so, libtfft_gcconv.so

def _context(r, a, ctx, behind, view):
    """a sequence [B][C][L] and its context [B][C][n] (`behind`: a future, else a history). view: the context as a view of the
    sequence's own far-strided buffer, `in - Hn` or `g + L`; else a tensor of its own with a stride of its own. Dense: always its
    own contiguous tensor. Returns (sequence view, context view, the context's stride option)."""
    a = np.asarray(a)
    seqs, length = a.shape[0] * a.shape[1], a.shape[2]
    if ctx is None:
        return _seq_in(r, a), None, 0
    ctx = np.asarray(ctx)
    n = ctx.shape[2]
    if r.far and view:
        base = r.region("in", n + length, 0)
        b_seq, b_ctx = (base, base + length) if behind else (base + n, base)
        v_seq = r.put(a.reshape(seqs, length), b_seq, r.stride("in", length))
        return v_seq, r.put(ctx.reshape(seqs, n), b_ctx, r.stride("in", n)), r.opt("in")
    v_seq = _seq_in(r, a)
    return v_seq, r.put(ctx.reshape(seqs, n), r.region("in", n, seqs * n), r.stride("in", n, extra=16)), r.opt("in", extra=16)


def _far_cconv(tf, pool, lay, view):
    name = f"{lay.name} {'view' if view else 'own buffer'}"

    def fwd(tf_, x, h, hist=None, launch_iters=0, history=None):
        def go(r):
            rows, channels, length = x.shape
            vx, vh, sh = _context(r, x, hist, False, view)
            plan = tf.TfftChunkedConvPlan(rows, channels, length, h.shape[1], 0, in_seq_stride=r.opt("in"), out_seq_stride=r.opt("out"), launch_iters=launch_iters,
                                          history=hist.shape[2] if hist is not None else (history or 0), hist_seq_stride=sh)
            plan.set_taps(_dev(h))
            plan.exec(vx, _seq_out(r, x.shape), vh)
            res = r.finish()
            plan.close()
            return (res[0],)

        return _bcl(both(pool, lay, go, what="cconv forward " + name)[0], x.shape)

    def dx(tf_, g, h, fut=None, launch_iters=0, future=None):
        def go(r):
            rows, channels, length = g.shape
            vg, vf, sf = _context(r, g, fut, True, view)
            plan = tf.TfftChunkedConvGradPlan(rows, channels, length, h.shape[1], 0, g_seq_stride=r.opt("in"), dx_seq_stride=r.opt("out"), launch_iters=launch_iters,
                                              future=fut.shape[2] if fut is not None else (future or 0), fut_seq_stride=sf)
            plan.set_taps(_dev(h))
            plan.input_grad(vg, _seq_out(r, g.shape), vf)
            res = r.finish()
            plan.close()
            return (res[0],)

        return _bcl(both(pool, lay, go, what="cconv input gradient " + name)[0], g.shape)

    def dh(tf_, x, g, taps, hist=None, partials=0, history=None, twice=False):
        def go(r):
            rows, channels, length = x.shape
            vx, vh, sh = _context(r, x, hist, False, view)
            vg = _seq_in(r, g)
            plan = tf.TfftChunkedConvGradPlan(rows, channels, length, taps, 0, x_seq_stride=r.opt("in"), g_seq_stride=r.opt("in"), partials=partials,
                                              history=hist.shape[2] if hist is not None else (history or 0), hist_seq_stride=sh)
            outs = []
            for _ in range(2 if twice else 1):
                buf = _f32_out(channels, taps)
                plan.tap_grad(vx, vg, buf[64:64 + channels * taps], vh)
                outs.append(_f32_read(buf, channels, taps)[0])
            r.finish()
            plan.close()
            return tuple(outs)

        res = both(pool, lay, go, what="cconv tap gradient " + name)
        return list(res) if twice else res[0]

    return fwd, dx, dh


@pytest.mark.parametrize("view", [True, False], ids=["view", "own"])
@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_cconv(tf, pool, layout, length, taps, view, monkeypatch):
    """forward with a history, input gradient with a future, tap gradient with a history; contexts of `halo` samples"""
    import test_gpu_cconv as tc

    lay = fl.LAYOUTS[layout]
    fwd, dx, dh = _far_cconv(tf, pool, lay, view)
    monkeypatch.setattr(tc, "run_fwd", fwd)
    monkeypatch.setattr(tc, "run_dx", dx)
    monkeypatch.setattr(tc, "run_dh", dh)
    halo = sr.geometry(length, taps)[0]
    tc.test_forward_with_history(tf, length, taps, lay.rows, lay.channels, halo, 0, "noise")
    tc.test_input_grad_with_future(tf, length, taps, lay.rows, lay.channels, halo, 0, "noise")
    tc.test_tap_grad_with_history(tf, length, taps, lay.rows, lay.channels, halo, 0, "noise")


def _far_gcconv(tf, pool, lay, view):
    name = f"{lay.name} {'view' if view else 'own buffer'}"

    def has(d):
        return d["pre"] is not None, d["post"] is not None

    def fwd(tf_, d, launch_iters=0, room=None):
        def go(r):
            rows, channels, length = d["x"].shape
            vx, vh, sh = _context(r, d["x"], d["hist"], False, view)
            vp, vph, sph = (None, None, 0) if d["pre"] is None else _context(r, d["pre"], d["pre_hist"], False, view)
            vq = None if d["post"] is None else _seq_in(r, d["post"])
            plan = tf.TfftGatedChunkedConvPlan(rows, channels, length, d["h"].shape[1], 0, pre_gate=has(d)[0], post_gate=has(d)[1], in_seq_stride=r.opt("in"),
                                               out_seq_stride=r.opt("out"), pre_seq_stride=r.opt("in") if has(d)[0] else 0,
                                               post_seq_stride=r.opt("in") if has(d)[1] else 0, launch_iters=launch_iters,
                                               history=d["hist"].shape[2] if d["hist"] is not None else (room or 0), hist_seq_stride=sh, pre_hist_seq_stride=sph)
            plan.set_taps(_dev(d["h"]), _dev(d["skip"]))
            plan.exec(vx, _seq_out(r, d["x"].shape), pre=vp, post=vq, hist=vh, pre_hist=vph)
            res = r.finish()
            plan.close()
            return (res[0],)

        return _bcl(both(pool, lay, go, what="gcconv forward " + name)[0], d["x"].shape)

    def dx(tf_, d, launch_iters=0, room=None, want_dpre=True):
        shape = d["gy"].shape

        def go(r):
            rows, channels, length = shape
            pre, post = has(d)
            vg, vf, sf = _context(r, d["gy"], d["fut"], True, view)
            vq, vqf, sqf = (None, None, 0) if not post else _context(r, d["post"], d["post_fut"], True, view)
            vx = _seq_in(r, d["x"]) if pre else None
            vp = _seq_in(r, d["pre"]) if pre else None
            with_dpre = pre and want_dpre
            plan = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, d["h"].shape[1], 0, pre_gate=pre, post_gate=post, gy_seq_stride=r.opt("in"),
                                                   post_seq_stride=r.opt("in") if post else 0, x_seq_stride=r.opt("in") if pre else 0,
                                                   pre_seq_stride=r.opt("in") if pre else 0, dx_seq_stride=r.opt("out"),
                                                   dpre_seq_stride=r.opt("out") if with_dpre else 0, launch_iters=launch_iters,
                                                   future=d["fut"].shape[2] if d["fut"] is not None else (room or 0), fut_seq_stride=sf, post_fut_seq_stride=sqf)
            plan.set_taps(_dev(d["h"]), _dev(d["skip"]))
            v_dx = _seq_out(r, shape)
            v_dpre = _seq_out(r, shape) if with_dpre else None
            plan.input_grad(vg, v_dx, post=vq, x=vx, pre=vp, dpre=v_dpre, future=vf, post_future=vqf)
            res = r.finish()
            plan.close()
            return res[0], (res[1] if with_dpre else None)

        res = both(pool, lay, go, what="gcconv input gradient " + name)
        return _bcl(res[0], shape), (None if res[1] is None else _bcl(res[1], shape))

    def dh(tf_, d, partials=0, room=None, twice=False):
        def go(r):
            rows, channels, length = d["x"].shape
            taps = d["h"].shape[1]
            pre, post = has(d)
            vx, vh, sh = _context(r, d["x"], d["hist"], False, view)
            vp, vph, sph = (None, None, 0) if not pre else _context(r, d["pre"], d["pre_hist"], False, view)
            vg = _seq_in(r, d["gy"])
            vq = _seq_in(r, d["post"]) if post else None
            plan = tf.TfftGatedChunkedConvGradPlan(rows, channels, length, taps, 0, pre_gate=pre, post_gate=post, x_seq_stride=r.opt("in"),
                                                   pre_seq_stride=r.opt("in") if pre else 0, gy_seq_stride=r.opt("in"), post_seq_stride=r.opt("in") if post else 0,
                                                   partials=partials, history=d["hist"].shape[2] if d["hist"] is not None else (room or 0),
                                                   hist_seq_stride=sh, pre_hist_seq_stride=sph)
            outs = []
            lo = 128 + channels * taps
            for _ in range(2 if twice else 1):
                buf = _f32_out(channels, taps)
                plan.tap_grad(vx, vg, buf[64:64 + channels * taps], pre=vp, post=vq, dskip=buf[lo:lo + channels], history=vh, pre_history=vph)
                outs += list(_f32_read(buf, channels, taps))
            r.finish()
            plan.close()
            return tuple(outs)

        res = both(pool, lay, go, what="gcconv tap gradient " + name)
        return [(res[0], res[1]), (res[2], res[3])] if twice else (res[0], res[1])

    return fwd, dx, dh


@pytest.mark.parametrize("view", [True, False], ids=["view", "own"])
@pytest.mark.parametrize("length,taps", LONG_SHAPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gcconv(tf, pool, layout, length, taps, view, monkeypatch):
    """both gates and a skip; the histories of x and of the pre gate, the futures of gy and of the post gate, `halo` samples each"""
    import test_gpu_gcconv as tg

    lay = fl.LAYOUTS[layout]
    fwd, dx, dh = _far_gcconv(tf, pool, lay, view)
    monkeypatch.setattr(tg, "run_fwd", fwd)
    monkeypatch.setattr(tg, "run_dx", dx)
    monkeypatch.setattr(tg, "run_dh", dh)
    halo = sr.geometry(length, taps)[0]
    args = (tf, length, taps, lay.rows, lay.channels, halo, 0, gc.EVERY_CASE_MODE, "noise")
    tg.test_forward_is_the_shipped_gated_plan_on_the_concatenated_sequences(*args)
    tg.test_input_grad_is_the_shipped_gated_plan_on_the_concatenated_sequences(*args)
    tg.test_tap_grad_is_the_shipped_gated_plan_on_the_concatenated_sequences(*args)


# =================================================================== libtfft_stft.so, _stftn.so, _istft.so, _istftn.so

def _stft_shape(n):
    """FRAME_ROWS signals of FRAMES_PER_ROW frames: (rows, length, hop, pad)"""
    return fl.FRAME_ROWS, n + n // 2, n // 2, 0


def _far_stft(tf, pool, lay, n, x, w, hop, pad):
    rows, length = x.shape
    bins, pitch = n // 2 + 1, (n // 2 + 1 + 7) // 8 * 8

    def go(r):
        kw = dict(in_sig_stride=r.opt("in"), out_frame_stride=r.opt("out"))
        plan = tf.TfftStftPlan(rows, length, hop, pad, 0, **kw) if n == st.N else tf.TfftShortStftPlan(n, rows, length, hop, pad, 0, **kw)
        assert plan.frames == fl.FRAMES_PER_ROW and plan.pitch == pitch
        plan.set_window(_dev(w))
        total = rows * plan.frames
        vx = r.put(x, r.region("in", length, rows * length), r.stride("in", length))
        b = r.region("out", 2 * pitch, total * 2 * pitch)
        o_re, o_im = r.out(total, bins, b, r.stride("out", 2 * pitch)), r.out(total, bins, b + pitch, r.stride("out", 2 * pitch))
        plan.exec(vx, o_re, o_im)
        res = r.finish()
        plan.close()
        return tuple(res)

    return both(pool, lay, go, {"in": rows, "out": SIX}, f"stft n={n} {lay.name}")


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stft(tf, pool, layout, n):
    """far in_sig_stride, far out_frame_stride: the shipped TfftRealPlan on host-built frames, bit for bit; fp64, frame by frame"""
    import test_gpu_stft as ts
    import test_gpu_stftn as tn

    lay = fl.LAYOUTS[layout]
    rows, length, hop, pad = _stft_shape(n)
    x, w = st.case_data(rows, length, window="random") if n == st.N else sn.case_data(n, rows, length, window="random")
    re, im = _far_stft(tf, pool, lay, n, x, w, hop, pad)
    what = f"stft n={n} R={rows} L={length} hop={hop} {layout}"
    if n == st.N:
        frames = st.frames(x, w, hop, pad)
        ts._assert_bits(what, (re, im), ts.via_real_plan(tf, frames))
    else:
        frames = sn.frames(x, w, hop, pad)
        tn._assert_bits(what, (re, im), tn.via_real_plan(tf, n, frames))
    got = re.view(np.float16).astype(np.float64) + 1j * im.view(np.float16).astype(np.float64)
    rounded = np.fft.rfft(frames.astype(np.float64), axis=-1) / n
    assert st.rel_l2(got, rounded).max() <= ts.K_RFFT, what


def _far_istft(tf, pool, lay, n, re, im, w, rows, length, hop, pad):
    bins, pitch = n // 2 + 1, (n // 2 + 1 + 7) // 8 * 8
    total = re.shape[0]
    poisoned = im.view(np.int16).copy()          # the IM of bins 0 and n / 2 must not be read
    poisoned[:, 0] = poisoned[:, n // 2] = fl.SENTINEL

    def go(r):
        kw = dict(in_frame_stride=r.opt("in"), out_sig_stride=r.opt("out"))
        plan = tf.TfftIstftPlan(rows, length, hop, pad, 0, **kw) if n == st.N else tf.TfftShortIstftPlan(n, rows, length, hop, pad, 0, **kw)
        assert rows * plan.frames == total
        plan.set_window(_dev(w))
        b = r.region("in", 2 * pitch, total * 2 * pitch)
        i_re, i_im = r.put(re.view(np.int16), b, r.stride("in", 2 * pitch)), r.put(poisoned, b + pitch, r.stride("in", 2 * pitch))
        vy = r.out(rows, length, r.region("out", length, rows * length), r.stride("out", length))
        plan.exec(i_re, i_im, vy)              # the workspace is the plan's own
        res = r.finish()
        plan.close()
        return tuple(res)

    return both(pool, lay, go, {"in": SIX, "out": rows}, f"istft n={n} {lay.name}")[0]


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_istft(tf, pool, layout, n):
    """far in_frame_stride, far out_sig_stride: the shipped inverse plan on the merged items, then the overlap-add of
    tests/istft_ref.py / istftn_ref.py on those frames, bit for bit"""
    import test_gpu_istft as ti
    import test_gpu_istftn as tn

    lay = fl.LAYOUTS[layout]
    rows, length, hop, pad = _stft_shape(n)
    what = f"istft n={n} R={rows} L={length} hop={hop} {layout}"
    if n == st.N:
        x, w = st.case_data(rows, length, window="random")
        re, im = ir.spectra16(x, w, hop, pad)
        y = _far_istft(tf, pool, lay, n, re, im, w, rows, length, hop, pad)
        frames = ti.via_inverse_plan(tf, *ir.merge_items(re, im), re.shape[0])
        want = ir.ola(frames.view(np.float16), w, rows, length, hop, pad).view(np.int16)
    else:
        x, w = sn.case_data(n, rows, length, window="random")
        re, im = inr.spectra16(x, w, hop, pad)
        y = _far_istft(tf, pool, lay, n, re, im, w, rows, length, hop, pad)
        frames = tn.via_inverse_plan(tf, n, *inr.merge_items(re, im, n), re.shape[0])
        want = inr.ola(frames.view(np.float16), w, n, rows, length, hop, pad).view(np.int16)
    assert np.isfinite(y.view(np.float16)).all(), what
    ti._assert_bits(what + ", output against the overlap-add of the shipped inverse plan's frames", y, want, ("signal", "sample"))


# =============================================================================================================== refusals

def _refusal_cases(tf):
    """name -> (make(stride_in, stride_out) -> plan, call(plan, x, y), halves per run in, out, counts): the smallest call of one
    plan per add-on group; x is the input tensor that the case hands over one half too short"""
    L, K, n = 4104, 7, 4096

    def taps(plan):
        plan.set_taps(torch.zeros(plan.channels * K, dtype=torch.float16, device=DEV))
        return plan

    def window(plan):
        plan.set_window(torch.ones(plan.n, dtype=torch.float16, device=DEV))
        return plan

    def flt(plan):
        z = torch.zeros(n, dtype=torch.float16, device=DEV)
        plan.set_filter(z, z)
        return plan

    return {
        "core": (lambda si, so: tf.TfftPlan(n, 3, 0, in_batch_stride=si, out_batch_stride=so, preserve_input=True),
                 lambda p, x, y: p.exec(x, x, y, y), n, n),
        "real": (lambda si, so: tf.TfftRealPlan(n, 3, 0, in_batch_stride=si, out_batch_stride=so), lambda p, x, y: p.r2c(x, y, y), n, n // 2 + 1),
        "conv": (lambda si, so: flt(tf.TfftConvPlan(n, 3, 1, 0, in_batch_stride=si, out_batch_stride=so)), lambda p, x, y: p.exec(x, x, y, y), n, n),
        "lconv": (lambda si, so: taps(tf.TfftCausalConvPlan(3, 1, 520, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), 520, 520),
        "gconv": (lambda si, so: taps(tf.TfftGatedConvPlan(3, 1, 520, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), 520, 520),
        "sconv": (lambda si, so: taps(tf.TfftLongConvPlan(3, 1, L, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), L, L),
        "gsconv": (lambda si, so: taps(tf.TfftGatedLongConvPlan(3, 1, L, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), L, L),
        "bconv": (lambda si, so: taps(tf.TfftLongConvGradPlan(3, 1, L, K, 0, g_seq_stride=si, dx_seq_stride=so)), lambda p, x, y: p.input_grad(x, y), L, L),
        "gbconv": (lambda si, so: taps(tf.TfftGatedLongConvGradPlan(3, 1, L, K, 0, gy_seq_stride=si, dx_seq_stride=so)), lambda p, x, y: p.input_grad(x, y), L, L),
        "cconv": (lambda si, so: taps(tf.TfftChunkedConvPlan(3, 1, L, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), L, L),
        "gcconv": (lambda si, so: taps(tf.TfftGatedChunkedConvPlan(3, 1, L, K, 0, in_seq_stride=si, out_seq_stride=so)), lambda p, x, y: p.exec(x, y), L, L),
        "stft": (lambda si, so: window(tf.TfftStftPlan(3, n, n, 0, 0, in_sig_stride=si, out_frame_stride=so)), lambda p, x, y: p.exec(x, y, y), n, n // 2 + 1),
        "stftn": (lambda si, so: window(tf.TfftShortStftPlan(512, 3, 512, 512, 0, 0, in_sig_stride=si, out_frame_stride=so)),
                  lambda p, x, y: p.exec(x, y, y), 512, 257),
        "istft": (lambda si, so: window(tf.TfftIstftPlan(3, n, n, 0, 0, in_frame_stride=si, out_sig_stride=so)), lambda p, x, y: p.exec(x, x, y), n // 2 + 1, n),
        "istftn": (lambda si, so: window(tf.TfftShortIstftPlan(512, 3, 512, 512, 0, 0, in_frame_stride=si, out_sig_stride=so)),
                   lambda p, x, y: p.exec(x, x, y), 257, 512),
    }


REFUSALS = ["core", "real", "conv", "lconv", "gconv", "sconv", "gsconv", "bconv", "gbconv", "cconv", "gcconv", "stft", "stftn", "istft", "istftn"]


@pytest.mark.parametrize("name", REFUSALS)
def test_an_arena_one_half_too_short_is_refused(tf, pool, name):
    """(count - 1) * stride + len - 1 halves at a far stride, on the input side and on the output side: the binding refuses, nothing
    is launched, both arenas are untouched. A stride narrowed to 32 bits on its way would make the short tensor long enough."""
    lay = fl.LAYOUTS["wide"]
    make, call, len_in, len_out = _refusal_cases(tf)[name]
    sizes = dict({side: fl.arena_halves(lay, side, 3) for side in fl.SIDES}, din=DENSE, dout=DENSE)
    short = pool.missing(sizes)
    if short:
        pytest.skip(f"needs {sum(sizes.values()) * 2 >> 30} GiB of HBM and {fl.Pool.HEADROOM >> 30} GiB of headroom: {short >> 20} MiB short")
    arenas = pool.get(sizes)
    b_in, b_out = fl.Block(0, 3, lay.in_stride, len_in), fl.Block(0, 3, lay.out_stride, len_out)
    x, y = _half(arenas["in"].view(b_in)), _half(arenas["out"].view(b_out))
    plan = make(lay.in_stride, lay.out_stride)
    for xs, ys in ((x[:-1], y), (x, y[:-1])):
        with pytest.raises(tf.TfftError, match="shorter"):
            call(plan, xs, ys)
    torch.cuda.synchronize()
    plan.close()
    for side in fl.SIDES:
        arenas[side].check_gaps(name)          # no block is placed: every half of both arenas

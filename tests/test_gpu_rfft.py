"""Real-input plans on the GPU (tfft_rplan_*, include/tfft.h): the split / merge kernels and the fused N = 4096 epilogue against the
library's own complex path plus the numpy restatement of the arithmetic (tests/rfft_ref.py, bit for bit), accuracy against float64
numpy, and the layout conventions."""
import numpy as np
import pytest

import rfft_ref
from tensor_fft_amd import capi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


DEV = "cuda:0"


def _signals(rng, batch, n, amp=1.0):
    return (rng.uniform(-1, 1, (batch, n)) * amp).astype(np.float16)


def _h16(t):
    return t.cpu().numpy().view(np.uint16)


def _r2c(tf, x, two_pass=False, **kw):
    """R2C of the (batch, n) fp16 array x in the default layout -> (re, im) fp16 arrays (batch, n/2 + 1)."""
    batch, n = x.shape
    plan = tf.TfftRealPlan(n, batch, 0, two_pass=two_pass, **kw)
    h = plan.pitch
    dx = torch.from_numpy(x).to(DEV).reshape(-1)
    out = torch.full((batch * 2 * h,), float("nan"), dtype=torch.float16, device=DEV)
    plan.r2c(dx, out, out[h:])
    torch.cuda.synchronize()
    o = out.cpu().numpy().reshape(batch, 2 * h)
    return o[:, :n // 2 + 1], o[:, h:h + n // 2 + 1]


def _c2r(tf, re, im, n, two_pass=False, **kw):
    batch = re.shape[0]
    plan = tf.TfftRealPlan(n, batch, 0, two_pass=two_pass, **kw)
    h = plan.pitch
    spec = np.zeros((batch, 2 * h), np.float16)
    spec[:, :n // 2 + 1] = re
    spec[:, h:h + n // 2 + 1] = im
    ds = torch.from_numpy(spec).to(DEV).reshape(-1)
    out = torch.empty(batch * n, dtype=torch.float16, device=DEV)
    plan.c2r(ds, ds[h:], out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(batch, n)


def _complex_pairs(tf, x, fused, scale="sequential"):
    """Z = the library's complex transform of the pairs of x, formed as the real plans form them: the batch // 2 full pairs by one
    plan over stride 2n, the odd last signal with itself by a plan of batch 1 (fused N = 4096: one plan over all pairs; the N =
    4096 kernel computes every transform alike). Returns fp16 (zr, zi) of shape (pairs, n)."""
    batch, n = x.shape
    pairs, full = (batch + 1) // 2, batch // 2
    dx = torch.from_numpy(x).to(DEV).reshape(-1)
    zr = torch.empty((pairs, n), dtype=torch.float16, device=DEV)
    zi = torch.empty((pairs, n), dtype=torch.float16, device=DEV)
    zb = torch.empty((pairs, 2 * n), dtype=torch.float16, device=DEV)
    flat = zb.reshape(-1)
    if fused or batch % 2 == 0:
        cnt = pairs if fused else full
        if batch % 2 and fused:
            xx = np.concatenate([x, x[-1:]])      # the self-paired last signal, as the fused kernel reads it
            dx = torch.from_numpy(xx).to(DEV).reshape(-1)
        p = tf.TfftPlan(n, cnt, 0, in_batch_stride=2 * n, preserve_input=True, scale=scale)
        p.exec(dx, dx[n:], flat, flat[n:])
    else:
        if full:
            p = tf.TfftPlan(n, full, 0, in_batch_stride=2 * n, preserve_input=True, scale=scale)
            p.exec(dx, dx[n:], flat, flat[n:])
        last = dx[(batch - 1) * n:].clone()
        t = tf.TfftPlan(n, 1, 0, preserve_input=True, scale=scale)
        tail = flat[full * 2 * n:]
        t.exec(last, last, tail, tail[n:])
    torch.cuda.synchronize()
    z = zb.cpu().numpy()
    return z[:, :n], z[:, n:]


def _expand(spec_pairs, batch):
    """Half spectra of the pairs (A of pair p = signal 2p, B = 2p + 1) -> per signal, the odd last signal taking its pair's A."""
    ar, ai, br, bi = spec_pairs
    pairs = ar.shape[0]
    re = np.empty((2 * pairs, ar.shape[1]), np.float16)
    im = np.empty_like(re)
    re[0::2], im[0::2], re[1::2], im[1::2] = ar, ai, br, bi
    return re[:batch], im[:batch]


def _merge_pairs(re, im, n):
    """numpy merge of the half spectra (batch, n/2 + 1) into the pairs' fp16 Z (pairs, n), pairs formed as the real plans form them."""
    a_idx, b_idx = rfft_ref.pair_rows(re.shape[0])
    return rfft_ref.merge(re[a_idx], im[a_idx], re[b_idx], im[b_idx], n)


def _complex_inverse_pairs(tf, zr, zi, batch, scale="sequential"):
    """The library's inverse complex transform of the pairs' Z, run as the real plans run it (the batch // 2 full pairs by one plan,
    the self-paired odd tail by a plan of batch 1). Returns (2 * pairs, n) fp16: row 2p the RE output of pair p, row 2p + 1 its IM."""
    pairs, n = zr.shape
    full = batch // 2
    zb = torch.from_numpy(np.concatenate([zr, zi], axis=1)).to(DEV).reshape(-1)
    out = torch.empty((pairs, 2 * n), dtype=torch.float16, device=DEV)
    flat = out.reshape(-1)
    if full:
        p = tf.TfftPlan(n, full, 0, preserve_input=True, scale=scale)
        p.exec_inverse(zb, zb[n:], flat, flat[n:])
    if batch % 2:
        t = tf.TfftPlan(n, 1, 0, preserve_input=True, scale=scale)
        zt = zb[full * 2 * n:].clone()
        ot = flat[full * 2 * n:]
        t.exec_inverse(zt, zt[n:], ot, ot[n:])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    rows = np.empty((2 * pairs, n), np.float16)
    rows[0::2], rows[1::2] = o[:, :n], o[:, n:]
    return rows


SIZES = [16, 256, 1024, 4096, 8192, 1 << 16, 1 << 20]
BATCHES = [1, 2, 3, 8, 65]


@pytest.mark.parametrize("n", SIZES)
def test_r2c_is_split_of_the_complex_path_bit_for_bit(tf, n):
    rng = np.random.default_rng(n)
    for batch in BATCHES:
        x = _signals(rng, batch, n)
        zr, zi = _complex_pairs(tf, x, fused=(n == 4096))
        want = _expand(rfft_ref.split(zr, zi), batch)
        got = _r2c(tf, x)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint16), w.view(np.uint16)), (n, batch)


@pytest.mark.parametrize("n", SIZES)
def test_c2r_is_inverse_of_the_merge_bit_for_bit(tf, n):
    rng = np.random.default_rng(n + 7)
    for batch in BATCHES:
        re = (rng.uniform(-1, 1, (batch, n // 2 + 1)) / 4).astype(np.float16)
        im = (rng.uniform(-1, 1, (batch, n // 2 + 1)) / 4).astype(np.float16)
        zr, zi = _merge_pairs(re, im, n)
        want = _complex_inverse_pairs(tf, zr, zi, batch)
        got = _c2r(tf, re, im, n)
        assert np.array_equal(got.view(np.uint16), want[:batch].view(np.uint16)), (n, batch)


@pytest.mark.parametrize("batch", [1, 2, 3, 4096, 131072])
def test_fused_r2c_equals_the_two_pass_path(tf, batch):
    rng = np.random.default_rng(batch)
    x = _signals(rng, batch, 4096)
    fused, two = tf.TfftRealPlan(4096, batch, 0), tf.TfftRealPlan(4096, batch, 0, two_pass=True)
    assert fused.num_launches() == 1 and two.num_launches() == 2 + (1 if batch % 2 and batch > 1 else 0)
    h = fused.pitch
    dx = torch.from_numpy(x).to(DEV).reshape(-1)
    o1 = torch.full((batch * 2 * h,), float("nan"), dtype=torch.float16, device=DEV)
    o2 = o1.clone()
    fused.r2c(dx, o1, o1[h:])
    two.r2c(dx, o2, o2[h:])
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))


def _rel_l2(got, want):
    return np.sqrt((np.abs(got - want) ** 2).sum(-1) / (np.abs(want) ** 2).sum(-1))


SCALE_DIV = {"sequential": lambda n: n, "once": lambda n: n, "none": lambda n: 1}


@pytest.mark.parametrize("scale", ["sequential", "none", "once"])
@pytest.mark.parametrize("n", [256, 4096, 1 << 16])
def test_r2c_accuracy_against_float64(tf, n, scale):
    rng = np.random.default_rng(3 * n)
    batch = 6
    x = _signals(rng, batch, n, amp=1.0 if scale != "none" else 8.0 / np.sqrt(n))
    re, im = _r2c(tf, x, scale=scale)
    div = SCALE_DIV[scale](n)
    want = np.fft.rfft(x.astype(np.float64), axis=-1) / div
    got = re.astype(np.float64) + 1j * im.astype(np.float64)
    assert (_rel_l2(got, want) <= 1.5e-3).all(), _rel_l2(got, want)
    # max error <= the complex path's max error on the same pair + 1 fp16 ulp of the pair's largest bin
    zr, zi = _complex_pairs(tf, x, fused=(n == 4096), scale=scale)
    a_idx, b_idx = rfft_ref.pair_rows(batch)
    zw = np.fft.fft(x[a_idx].astype(np.float64) + 1j * x[b_idx].astype(np.float64), axis=-1) / div
    zerr = np.abs(zr.astype(np.float64) + 1j * zi.astype(np.float64) - zw).max(-1)
    top = np.abs(zw).max(-1)
    ulp = 2.0 ** (np.floor(np.log2(top)) - 10)
    for s in range(batch):
        p = s // 2
        assert np.abs(got[s] - want[s]).max() <= zerr[p] + ulp[p], (s, np.abs(got[s] - want[s]).max(), zerr[p], ulp[p])


def test_fused_path_ignores_plan_wisdom(tf):
    """A wisdom line may give a variant-0 N = 4096 complex plan another decomposition (AUTOSORT_ONLY: the plain autosort chain, no
    N = 4096 kernel and no tables). The real plans pin their forward sub-plans to the N = 4096 kernel: the fused launch still finds
    its tables, and fused and two-pass R2C still agree bit for bit, with each other and with the result without wisdom."""
    rng = np.random.default_rng(21)
    x = _signals(rng, 5, 4096)
    plain = _r2c(tf, x)
    tf.tuning_add(4096, 0, capi.VARIANT_AUTOSORT_ONLY, 0)
    try:
        assert tf.plan_describe(4096, 1, tf.plan_default_variant(4096, 1, 3)).startswith("autosort")
        assert tf.rplan_describe(4096, 5).startswith("r2c: k4096:4096+split | c2r: merge autosort")
        fused = _r2c(tf, x)
        two = _r2c(tf, x, two_pass=True)
    finally:
        tf.tuning_clear()
    for a, b, c in zip(plain, fused, two):
        assert np.array_equal(a.view(np.uint16), b.view(np.uint16)) and np.array_equal(a.view(np.uint16), c.view(np.uint16))


def test_mismatched_pair_meets_the_pair_relative_bound(tf):
    n = 4096
    rng = np.random.default_rng(11)
    x = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n) * 1e-3]).astype(np.float16)
    re, im = _r2c(tf, x)
    want = np.fft.rfft(x.astype(np.float64), axis=-1) / n
    got = re.astype(np.float64) + 1j * im.astype(np.float64)
    pair_top = np.abs(np.fft.fft(x[0].astype(np.float64) + 1j * x[1].astype(np.float64)) / n).max()
    # documented bound (include/tfft.h): relative to the pair's largest bin; the quiet signal's own relative error is NOT small
    assert np.abs(got - want).max() <= 2e-3 * pair_top
    assert _rel_l2(got[:1], want[:1])[0] <= 1.5e-3


@pytest.mark.parametrize("scale", ["sequential", "none", "once"])
@pytest.mark.parametrize("n", [256, 4096, 1 << 16])
def test_c2r_accuracy_against_float64(tf, n, scale):
    rng = np.random.default_rng(5 * n)
    batch = 5
    amp = 1.0 / n if scale == "none" else 1.0
    X = (rng.uniform(-1, 1, (batch, n // 2 + 1)) + 1j * rng.uniform(-1, 1, (batch, n // 2 + 1))) * amp
    re, im = X.real.astype(np.float16), X.imag.astype(np.float16)
    got = _c2r(tf, re, im, n, scale=scale).astype(np.float64)
    Xq = re.astype(np.float64) + 1j * im.astype(np.float64)
    c = n / SCALE_DIV[scale](n)                   # the inverse's factor beyond numpy's 1/n (n for an unscaled plan)
    want = np.fft.irfft(Xq, n, axis=-1) * c
    assert (_rel_l2(got, want) <= 1.5e-3).all(), _rel_l2(got, want)
    # max error <= the complex path's max error on the same pair + 1 fp16 ulp of the pair's largest bin (carried through the
    # inverse: times c). The merged Z is rfft_ref.merge's (the bit-for-bit test above pins the kernel to it); its rounding moves
    # each bin by at most half an ulp per component, which the inverse turns into at most c ulp of the largest bin.
    zr, zi = _merge_pairs(re, im, n)
    zq = zr.astype(np.float64) + 1j * zi.astype(np.float64)
    lib = _complex_inverse_pairs(tf, zr, zi, batch, scale=scale).astype(np.float64)
    exact = np.fft.ifft(zq, axis=-1) * c
    pairs = zq.shape[0]
    zerr = np.maximum(np.abs(lib[0::2] - exact.real).max(-1), np.abs(lib[1::2] - exact.imag).max(-1))
    top = np.abs(zq).max(-1)
    ulp = 2.0 ** (np.floor(np.log2(top)) - 10)
    assert zerr.shape == (pairs,)
    for s in range(batch):
        p = s // 2
        err = np.abs(got[s] - want[s]).max()
        assert err <= zerr[p] + c * ulp[p], (s, err, zerr[p], c * ulp[p])


@pytest.mark.parametrize("n", [16, 4096, 8192])
def test_round_trip_is_x_over_n(tf, n):
    rng = np.random.default_rng(n + 3)
    x = _signals(rng, 7, n)
    re, im = _r2c(tf, x)
    y = _c2r(tf, re, im, n).astype(np.float64)
    assert (_rel_l2(y, x.astype(np.float64) / n) <= 3e-3).all()


def test_torch_convenience_matches_the_plan(tf):
    rng = np.random.default_rng(2)
    x = _signals(rng, 5, 1024)
    dx = torch.from_numpy(x).to(DEV)
    re, im = tf.rfft(dx)
    assert re.shape == (5, 513) and im.shape == (5, 513)
    w_re, w_im = _r2c(tf, x)
    assert np.array_equal(_h16(re), w_re.view(np.uint16)) and np.array_equal(_h16(im), w_im.view(np.uint16))
    y = tf.irfft(re, im, 1024)
    assert y.shape == (5, 1024)
    assert np.array_equal(_h16(y), _c2r(tf, w_re, w_im, 1024).view(np.uint16))


@pytest.mark.parametrize("n", [64, 4096, 1 << 16])
def test_strided_layout_leaves_every_other_byte_alone(tf, n):
    rng = np.random.default_rng(n + 9)
    batch, rs, ss = 5, n + 24, n // 2 + 1 + 40
    ss += (-ss) % 8
    bins = n // 2 + 1
    x = _signals(rng, batch, n)
    xs = np.full((batch, rs), np.float16(np.nan))
    xs[:, :n] = x
    dx = torch.from_numpy(xs).to(DEV).reshape(-1)
    nan = float("nan")
    o_re = torch.full((batch * ss,), nan, dtype=torch.float16, device=DEV)
    o_im = torch.full((batch * ss,), nan, dtype=torch.float16, device=DEV)
    plan = tf.TfftRealPlan(n, batch, 0, in_batch_stride=rs, out_batch_stride=ss)
    plan.r2c(dx, o_re, o_im)
    y = torch.full((batch * rs,), nan, dtype=torch.float16, device=DEV)
    plan.c2r(o_re, o_im, y)
    torch.cuda.synchronize()
    re, im = (t.cpu().numpy().reshape(batch, ss) for t in (o_re, o_im))
    w_re, w_im = _r2c(tf, x)
    assert np.array_equal(re[:, :bins].view(np.uint16), w_re.view(np.uint16))
    assert np.array_equal(im[:, :bins].view(np.uint16), w_im.view(np.uint16))
    assert np.isnan(re[:, bins:]).all() and np.isnan(im[:, bins:]).all()
    yy = y.cpu().numpy().reshape(batch, rs)
    assert np.array_equal(yy[:, :n].view(np.uint16), _c2r(tf, w_re, w_im, n).view(np.uint16))
    assert np.isnan(yy[:, n:]).all()
    # the default layout never writes the pitch padding either
    o = torch.full((batch * 2 * plan.pitch,), nan, dtype=torch.float16, device=DEV)
    p2 = tf.TfftRealPlan(n, batch, 0)
    p2.r2c(torch.from_numpy(x).to(DEV).reshape(-1), o, o[plan.pitch:])
    oo = o.cpu().numpy().reshape(batch, 2, plan.pitch)
    assert np.isnan(oo[:, :, bins:]).all() and not np.isnan(oo[:, :, :bins]).any()


@pytest.mark.parametrize("n", [256, 4096, 1 << 16])
def test_c2r_ignores_imaginary_part_of_edge_bins_and_inputs_stay_unchanged(tf, n):
    rng = np.random.default_rng(n + 13)
    batch = 3
    x = _signals(rng, batch, n)
    plan = tf.TfftRealPlan(n, batch, 0)
    h = plan.pitch
    dx = torch.from_numpy(x).to(DEV).reshape(-1)
    x0 = dx.clone()
    spec = torch.zeros(batch * 2 * h, dtype=torch.float16, device=DEV)
    plan.r2c(dx, spec, spec[h:])
    s0 = spec.clone()
    y1 = torch.empty(batch * n, dtype=torch.float16, device=DEV)
    plan.c2r(spec, spec[h:], y1)
    torch.cuda.synchronize()
    assert torch.equal(dx.view(torch.int16), x0.view(torch.int16))
    assert torch.equal(spec.view(torch.int16), s0.view(torch.int16))
    s = spec.view(batch, 2 * h)
    s[:, h] = 3.0
    s[:, h + n // 2] = -5.0
    y2 = torch.empty_like(y1)
    plan.c2r(spec, spec[h:], y2)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))


@pytest.mark.parametrize("n, two_pass", [(4096, False), (4096, True), (1 << 20, False)])
def test_prepared_plan_is_launches_only_and_replays_under_a_graph(tf, n, two_pass):
    """After prepare() the first executions happen under stream capture, where an allocation would fail the capture; the replay
    gives the bits of eager executions, and a caller's workspace gives the same bits again."""
    rng = np.random.default_rng(n)
    batch = 9
    plan = tf.TfftRealPlan(n, batch, 0, two_pass=two_pass)
    assert plan.workspace_bytes >= ((batch + 1) // 2) * n * 4
    plan.prepare()
    h = plan.pitch
    dx = torch.from_numpy(_signals(rng, batch, n)).to(DEV).reshape(-1)
    spec = torch.zeros(batch * 2 * h, dtype=torch.float16, device=DEV)
    y = torch.zeros(batch * n, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        plan.r2c(dx, spec, spec[h:])
        plan.c2r(spec, spec[h:], y)
    g.replay()
    torch.cuda.synchronize()
    got_s, got_y = spec.clone(), y.clone()
    want_s = torch.zeros_like(spec)        # (the pitch padding is never written: same zeros in every buffer compared)
    want_y = torch.empty_like(y)
    plan.r2c(dx, want_s, want_s[h:])
    plan.c2r(want_s, want_s[h:], want_y)
    torch.cuda.synchronize()
    assert torch.equal(got_s.view(torch.int16), want_s.view(torch.int16))
    assert torch.equal(got_y.view(torch.int16), want_y.view(torch.int16))
    own = tf.TfftRealPlan(n, batch, 0, two_pass=two_pass)
    own.set_workspace(torch.empty(own.workspace_bytes, dtype=torch.uint8, device=DEV))
    s2, y2 = torch.zeros_like(spec), torch.empty_like(y)
    own.r2c(dx, s2, s2[h:])
    own.c2r(s2, s2[h:], y2)
    torch.cuda.synchronize()
    assert torch.equal(s2.view(torch.int16), want_s.view(torch.int16)) and torch.equal(y2.view(torch.int16), want_y.view(torch.int16))


def test_pointer_checks(tf):
    plan = tf.TfftRealPlan(4096, 2, 0)
    h = plan.pitch
    buf = torch.zeros(2 * 4096 + 2 * 2 * h, dtype=torch.float16, device=DEV)
    x, spec = buf[:8192], buf[8192:]
    with pytest.raises(tf.TfftError):
        plan.r2c_ptr(x.data_ptr(), x.data_ptr(), x.data_ptr() + 2 * h * 2)         # in place
    with pytest.raises(tf.TfftError):
        plan.r2c_ptr(x.data_ptr() + 2, spec.data_ptr(), spec.data_ptr() + 2 * h)     # misaligned
    with pytest.raises(tf.TfftError):
        plan.r2c_ptr(x.data_ptr(), spec.data_ptr(), spec.data_ptr())                 # RE and IM planes identical
    with pytest.raises(tf.TfftError):
        plan.c2r_ptr(spec.data_ptr(), spec.data_ptr() + 2 * h, spec.data_ptr())      # output on the spectrum
    plan.r2c_ptr(x.data_ptr(), spec.data_ptr(), spec.data_ptr() + 2 * h, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

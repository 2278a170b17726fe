"""Workspace life cycles of a plan: prepare, stream capture, in-place execution after out of place, several executions in a row.

The kernel matrix checks every kernel under one life cycle: a fresh plan, one execution, a synchronise. Here the state a plan keeps
between calls is the subject, its workspace: who allocated it, how large it is, whether a later call may move it. The rules
(include/tfft.h, DESIGN.md "Workspace life cycle"):

    R1  once a plan is prepared, or any execution of it has returned, no tfft_exec / tfft_exec_inverse allocates or frees
    R2  in place gives the bits of out of place; on a library-owned workspace without the leading stockham::copy_kernel
    R3  tfft_plan_workspace_bytes() is one block, what a caller hands in; twice that enables the two-block chain

They are observed from outside: an allocation or a free under stream capture fails the capture (a host error, nothing faulty is
launched: no graph is replayed before every capture of its test has succeeded), and a workspace that moved, a sub-plan whose scratch was
not bound, or a pass on another stream shows in the bits. Every result is checked against fp64 with tests/elementwise_bound.py
and the project's constants; two runs of one plan are compared bit for bit. Input: seeded uniform(-1, 1) binary16, different for
every transform. Each test asserts the pass structure it relies on, so a planner change fails here loudly.

The shapes are the smallest at which each property exists (tfft_plan_describe):
    auto-3   n = 512 x 3, AUTOSORT_ONLY   autosort:16 autosort:16 autosort:2: the smallest chain with an odd number >= 3 of passes
    lat-3    n = 2^17 x 1                 col:256+tw col:256+tw autosort:2-tw: the latency kernels, the C++ shim's in-place case
    col-3    n = 2^21 x 8                 col:512+tw col:512+tw autosort:8-tw: the throughput three-pass chain
    col-2    n = 2^16 x 3                 col:256+tw col:256: the even control, whose own workspace stays one block
    tr-out / tr-in  n = 2^16 x 3          transposed output / input order: the chunk workspace between two sub-plans
    2d-rows  8 x 65536 x 2, 2d-cols 65536 x 16 x 2: a row / column sub-plan with scratch of its own behind the intermediate
    conv-2^16  (2^16, 5 signals, 2 filters): the composed path, two transposed sub-plans sharing one scratch share
    real-2^18  2^18 x 3: an odd batch, tail sub-plans and the scratch plane
    real-4096  4096 x 3: the fused real plan, one launch and no workspace

Section 7 is about the other state between calls: how the launch logic runs. tfft_plan_kernels & co. walk the launch logic of an
execution without launching; neither a walk that succeeds, nor one that fails half way, nor one on another thread may change what
the next execution launches.
"""
import ctypes

import numpy as np
import pytest

import conv_ref
import dist_emulate as de
import elementwise_bound as eb
from test_gpu_kernel_matrix import k_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
COPY = "stockham::copy_kernel"
G = de.GUARD


@pytest.fixture(scope="module")
def tf():
    import __graft_entry__ as g

    g.build()
    import tensor_fft_amd

    assert torch.cuda.is_available()
    tensor_fft_amd.device_check(0)
    return tensor_fft_amd


def _shapes(tf):
    a = tf.capi.VARIANT_AUTOSORT_ONLY
    return {
        "auto-3": dict(n=512, batch=3, variant=a, chain="autosort:16 autosort:16 autosort:2"),
        "lat-3": dict(n=1 << 17, batch=1, chain="col:256+tw col:256+tw autosort:2-tw"),
        "col-3": dict(n=1 << 21, batch=8, chain="col:512+tw col:512+tw autosort:8-tw"),
        "col-2": dict(n=1 << 16, batch=3, chain="col:256+tw col:256"),
        "tr-out": dict(n=1 << 16, batch=3, output_order="transposed"),
        "tr-in": dict(n=1 << 16, batch=3, input_order="transposed"),
    }


def make_plan(tf, sid, preserve_input=True):
    """The plan of a shape, with the pass structure the tests rely on asserted."""
    s = dict(_shapes(tf)[sid])
    chain = s.pop("chain", None)
    n, batch = s.pop("n"), s.pop("batch")
    plan = tf.TfftPlan(n, batch, 0, preserve_input=preserve_input, **s)
    if chain:
        variant = s.get("variant") or tf.capi.plan_default_variant(n, 1, batch)
        assert tf.plan_describe(n, 1, variant) == chain, sid
        assert plan.num_launches == len(chain.split()), (sid, plan.kernels)
        assert plan.workspace_bytes == batch * n * 4                    # R3: one block
    else:
        assert plan.num_launches == 2 and plan.workspace_bytes > 0, (sid, plan.kernels)      # sub_col + sub_row, chunk workspace
    return plan


# ---- seeded inputs and their fp64 references, computed once per (shape, input number) and never modified
_DATA = {}


def _data(tf, sid, k=0):
    """(x [batch][2][n] binary16 in the plan's input layout, fp64 forward spectrum / n in the plan's output layout, fp64 inverse)"""
    key = (sid, k)
    if key not in _DATA:
        s = _shapes(tf)[sid]
        n, batch = s["n"], s["batch"]
        rng = np.random.default_rng([20, n, batch, k, sorted(_shapes(tf)).index(sid)])
        x = rng.uniform(-1, 1, (batch, 2, n)).astype(np.float16)
        xc = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
        fwd = np.fft.fft(xc, axis=1) / n
        n2 = tf.transposed_n2(n)
        xin = x
        if s.get("input_order"):              # x[p + N1 q] at q + N2 p
            xin = np.ascontiguousarray(x.reshape(batch, 2, n2, n // n2).transpose(0, 1, 3, 2)).reshape(batch, 2, n)
        if s.get("output_order"):             # X[k1 + N1 k2] at k1 N2 + k2
            fwd = np.ascontiguousarray(fwd.reshape(batch, n2, n // n2).transpose(0, 2, 1)).reshape(batch, n)
        for a in (xin, fwd):
            a.setflags(write=False)
        _DATA[key] = (xin, fwd, xc)
    return _DATA[key]


def _inverse_ref(tf, sid, k=0):
    key = (sid, k, "inv")
    if key not in _DATA:
        _DATA[key] = np.fft.ifft(_data(tf, sid, k)[2], axis=1)
        _DATA[key].setflags(write=False)
    return _DATA[key]


def _dev(x):
    return torch.from_numpy(np.array(x).reshape(-1)).to(DEV)            # (a copy: the shared arrays are read-only)


def _bits(t):
    return t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(flat, ref, batch, n, k, what):
    got = flat.cpu().numpy().reshape(batch, 2, n).astype(np.float64)
    worst = eb.check(got[:, 0], got[:, 1], ref.real, ref.imag, k, rel_l2=eb.REL_L2, what=what)
    print(f"{what}: worst {worst:.3f} ulp (K = {k})")
    return worst


def _capture(fn):
    """fn() recorded on a side stream into a graph. An allocation, a free or a synchronise inside fn is a host error here."""
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fn()
    return graph


def _replay(graph):
    graph.replay()
    torch.cuda.synchronize()


def _guarded_workspace(nbytes):
    """(the whole buffer, the nbytes in its middle): a caller's workspace between guard zones"""
    assert nbytes % 2 == 0
    buf = de._guarded(torch, nbytes // 2)
    return buf, buf[G:G + nbytes // 2]


# ---------------------------------------------------------------------------------------------------------------------
# 1. prepared plan: the first executions happen under capture, out of place and in place
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["auto-3", "lat-3", "col-3", "col-2"])
def test_prepared_plan_first_executions_under_capture(tf, sid):
    """prepare(), no warm-up. Graph A: out of place; graph B: in place on a clone. Replays A, B, A: every A against fp64 and the
    same bits every time, B the bits of A. An in-place execution that allocates a second block (or frees the first) fails its
    capture; nothing is replayed before both captures have succeeded, so no graph with a stale pointer is ever launched."""
    plan = make_plan(tf, sid)
    n, batch = plan.n, plan.batch
    xin, fwd, _ = _data(tf, sid)
    k = k_of(plan.kernels, {"kind": "c"})
    plan.prepare()
    assert COPY not in plan.kernels_in_place                             # R2: the library's own workspace needs no copy
    x, y = _dev(xin), torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
    work = x.clone()
    graph_a = _capture(lambda: plan.exec(x, x[n:], y, y[n:]))
    graph_b = _capture(lambda: plan.exec(work, work[n:], work, work[n:]))
    _replay(graph_a)
    first = y.clone()
    _check(first, fwd, batch, n, k, f"{sid}: graph A, first replay")
    assert np.array_equal(x.cpu().numpy().view(np.int16), xin.reshape(-1).view(np.int16)), "input written (preserve_input)"
    _replay(graph_b)
    assert _same(work, first), "in place differs from out of place"
    y.zero_()
    _replay(graph_a)
    _check(y, fwd, batch, n, k, f"{sid}: graph A, replay after the in-place graph")
    assert _same(y, first), "second replay of the out-of-place graph differs from the first"
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. unprepared plan: the workspace the first (out-of-place) execution allocated serves every later one where it is
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["auto-3", "lat-3", "col-3"])
def test_first_execution_allocates_for_every_later_one(tf, sid):
    """Fresh plan, eager out-of-place execution: the library allocates. The in-place execution that follows is captured (R1: no
    second allocation, nothing freed), so is an out-of-place inverse; both replay to the right values, in place bit-identical
    to out of place and without the copy. Then the same with preserve_input = 0, where the first execution uses no workspace."""
    plan = make_plan(tf, sid)
    n, batch = plan.n, plan.batch
    xin, fwd, _ = _data(tf, sid)
    k = k_of(plan.kernels, {"kind": "c"})
    x, y = _dev(xin), torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
    plan.exec(x, x[n:], y, y[n:])
    torch.cuda.synchronize()
    _check(y, fwd, batch, n, k, f"{sid}: eager, out of place")
    work, z = x.clone(), torch.zeros_like(y)
    graph_in_place = _capture(lambda: plan.exec(work, work[n:], work, work[n:]))
    graph_inverse = _capture(lambda: plan.exec_inverse(x, x[n:], z, z[n:]))
    assert COPY not in plan.kernels_in_place
    _replay(graph_in_place)
    _replay(graph_inverse)
    assert _same(work, y), "in place differs from out of place"
    _check(z, _inverse_ref(tf, sid), batch, n, k, f"{sid}: captured inverse")
    plan.close()
    # the library's default, preserve_input = 0: the eager out-of-place execution takes its input as scratch (a copy here: the
    # shared input stays as it is) and uses no workspace itself, yet it settles the one the captured in-place execution needs
    plan = make_plan(tf, sid, preserve_input=False)
    scratch_in, y0 = x.clone(), torch.zeros_like(y)
    plan.exec(scratch_in, scratch_in[n:], y0, y0[n:])
    torch.cuda.synchronize()
    _check(y0, fwd, batch, n, k, f"{sid}: preserve_input = 0, eager, out of place")
    assert _same(y0, y), "preserve_input = 0 gives other bits"
    work0 = x.clone()
    graph_in_place0 = _capture(lambda: plan.exec(work0, work0[n:], work0, work0[n:]))
    assert COPY not in plan.kernels_in_place
    _replay(graph_in_place0)
    assert _same(work0, y), "preserve_input = 0: in place differs from out of place"
    plan.close()


@pytest.mark.parametrize("preserve_input", [True, False], ids=["preserve", "input-as-scratch"])
def test_single_strided_pass_settles_its_workspace_out_of_place(tf, preserve_input):
    """n = 256 along a strided axis of 16 columns, batch 3: one column pass that is no single kernel. Out of place it uses no
    scratch, in place one block (the chain starts from a copy). The eager out-of-place execution still settles the workspace
    (R1), so the in-place execution after it is captured; it gives the out-of-place bits."""
    n, inner, batch = 256, 16, 3
    nf = n * inner
    assert tf.plan_describe(n, inner, 0).count(":") == 1
    plan = tf.TfftPlan(n, batch, 0, inner=inner, preserve_input=preserve_input)
    assert plan.num_launches == 1 and plan.workspace_bytes == batch * nf * 4, plan.kernels
    assert plan.kernels_in_place[0] == COPY and len(plan.kernels_in_place) == 2
    rng = np.random.default_rng([25, n, inner, batch])
    xh = rng.uniform(-1, 1, (batch, 2, nf)).astype(np.float16)
    xc = (xh[:, 0].astype(np.float64) + 1j * xh[:, 1].astype(np.float64)).reshape(batch, n, inner)
    ref = (np.fft.fft(xc, axis=1) / n).reshape(batch, nf)
    x, y = _dev(xh), torch.zeros(batch * 2 * nf, dtype=torch.float16, device=DEV)
    src = x.clone()
    plan.exec(src, src[nf:], y, y[nf:])
    torch.cuda.synchronize()
    _check(y, ref, batch, nf, k_of(plan.kernels, {"kind": "c"}), f"256 x {inner} columns x {batch}: eager, out of place")
    work = x.clone()
    graph = _capture(lambda: plan.exec(work, work[nf:], work, work[nf:]))
    _replay(graph)
    assert _same(work, y), "in place differs from out of place"
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a caller's workspace of one block (chain from a copy) and of two (no copy), under capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["auto-3", "lat-3", "col-3"])
def test_caller_workspaces_under_capture(tf, sid):
    plan = make_plan(tf, sid)
    n, batch = plan.n, plan.batch
    xin, fwd, _ = _data(tf, sid)
    k = k_of(plan.kernels, {"kind": "c"})
    x = _dev(xin)
    block = plan.workspace_bytes
    # one block: out of place (the bits everything below is compared with), in place through the copy, forward and inverse
    buf1, ws1 = _guarded_workspace(block)
    plan.set_workspace(ws1)
    assert plan.kernels_in_place[0] == COPY and COPY not in plan.kernels_in_place[1:] and COPY not in plan.kernels
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    plan.exec(x, x[n:], y, y[n:])
    plan.exec_inverse(x, x[n:], z, z[n:])
    torch.cuda.synchronize()
    _check(y, fwd, batch, n, k, f"{sid}: caller's block, out of place")
    _check(z, _inverse_ref(tf, sid), batch, n, k, f"{sid}: caller's block, inverse out of place")
    work, work_inv = x.clone(), x.clone()
    graph_fwd = _capture(lambda: plan.exec(work, work[n:], work, work[n:]))
    graph_inv = _capture(lambda: plan.exec_inverse(work_inv, work_inv[n:], work_inv, work_inv[n:]))
    _replay(graph_fwd)
    _replay(graph_inv)
    assert _same(work, y), "one block: in place differs from out of place"
    assert _same(work_inv, z), "one block: in-place inverse differs from the out-of-place inverse"
    assert de._guards_intact(torch, buf1), "written outside the caller's block"
    # two blocks: IN -> A -> B -> IN, no copy
    buf2, ws2 = _guarded_workspace(2 * block)
    plan.set_workspace(ws2)
    assert COPY not in plan.kernels_in_place
    work2, work2_inv = x.clone(), x.clone()
    graph_fwd2 = _capture(lambda: plan.exec(work2, work2[n:], work2, work2[n:]))
    graph_inv2 = _capture(lambda: plan.exec_inverse(work2_inv, work2_inv[n:], work2_inv, work2_inv[n:]))
    _replay(graph_fwd2)
    _replay(graph_inv2)
    assert _same(work2, y), "two blocks: in place differs from out of place"
    assert _same(work2_inv, z), "two blocks: in-place inverse differs from the out-of-place inverse"
    assert de._guards_intact(torch, buf2), "written outside the caller's two blocks"
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. three executions of one plan in a row on one side stream, one synchronise at the end
# ---------------------------------------------------------------------------------------------------------------------
def _conv_plan(tf, n, batch, filters, h_re, h_im):
    plan = tf.TfftConvPlan(n, batch, filters, 0)
    plan.set_filter(_dev(h_re), _dev(h_im))
    return plan


def _conv_case(k=0):
    n, batch, filters = 1 << 16, 5, 2
    key = ("conv", k)
    if key not in _DATA:
        rng = np.random.default_rng([21, n, batch, filters, k])
        x_re, x_im = conv_ref.signals(n, batch, rng)
        if ("conv", "filter") not in _DATA:
            _DATA[("conv", "filter")] = conv_ref.to_half_planes(conv_ref.make_filters("allpass", n, filters, np.random.default_rng([22, n, filters])))
        h_re, h_im = _DATA[("conv", "filter")]
        r_re, r_im = conv_ref.reference(x_re, x_im, h_re, h_im)
        x = np.stack([x_re, x_im], axis=1)                      # [batch][RE n | IM n]
        x.setflags(write=False)
        _DATA[key] = (x, r_re + 1j * r_im)
    return (n, batch, filters) + _DATA[key] + _DATA[("conv", "filter")]


def _assert_conv_structure(plan):
    ks = plan.kernels
    assert plan.num_launches == len(ks) == 5 and ks[2] == "cmul::cmul_kernel", ks       # two transposed sub-plans of two passes
    assert plan.workspace_bytes > plan.batch * plan.n * 4, "no sub-plan scratch behind the spectra"


@pytest.mark.parametrize("sid", ["auto-3", "col-3", "tr-out", "tr-in", "conv-2^16"])
def test_back_to_back_executions_on_one_side_stream(tf, sid):
    """Three inputs, three outputs, one plan, one non-default stream, no synchronise in between. The plan's one workspace is
    protected by stream order alone: a pass or a copy on another stream, or on the default one, shows as a wrong output. Each output
    against fp64, and bit-identical to the same input run alone."""
    if sid == "conv-2^16":
        n, batch, _, _, _, h_re, h_im = _conv_case()
        plan = _conv_plan(tf, n, batch, 2, h_re, h_im)
        _assert_conv_structure(plan)
        cases = [_conv_case(i)[3:5] for i in range(3)]
        k = conv_ref.K_CONV_COMPOSED
    else:
        plan = make_plan(tf, sid)
        n, batch = plan.n, plan.batch
        cases = [_data(tf, sid, i)[:2] for i in range(3)]
        k = k_of(plan.kernels, {"kind": "c"})
    xs = [_dev(c[0]) for c in cases]
    ys = [torch.zeros_like(x) for x in xs]
    torch.cuda.synchronize()                       # the inputs are on the device before the side stream starts
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for x, y in zip(xs, ys):
            plan.exec(x, x[n:], y, y[n:])
    stream.synchronize()
    for i, (x, y) in enumerate(zip(xs, ys)):
        _check(y, cases[i][1], batch, n, k, f"{sid}: execution {i} of three in a row")
        alone = torch.zeros_like(y)
        plan.exec(x, x[n:], alone, alone[n:])
        torch.cuda.synchronize()
        assert _same(y, alone), f"execution {i} of three in a row differs from the same input run alone"
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. 2D plans whose sub-plans have scratch of their own
# ---------------------------------------------------------------------------------------------------------------------
def _exec2d_c(tf, plan, re, im, o_re, o_im):
    """tfft_plan2d_exec itself on the current stream: TfftPlan2D.exec would hand torch scratch in first"""
    stream = torch.cuda.current_stream(0).cuda_stream
    tf.capi._check(plan._lib.tfft_plan2d_exec(plan._h, re.data_ptr(), im.data_ptr(), o_re.data_ptr(), o_im.data_ptr(), stream))


@pytest.mark.parametrize("rows,cols,batch,row_chain,col_chain", [
    (8, 65536, 2, "col:256+tw col:256", "autosort:8"),            # 2d-rows: the row sub-plan has two passes
    (65536, 16, 2, "autosort:16", "col:256+tw col:256"),          # 2d-cols: the column sub-plan has two column passes
], ids=["2d-rows", "2d-cols"])
def test_2d_plans_with_sub_plan_scratch(tf, rows, cols, batch, row_chain, col_chain):
    """First execution under capture with a caller's workspace of exactly workspace_bytes (between guard zones), then the library's
    own allocation on a second plan (first execution eager, then captured): fft2 / (rows cols) element by element, and the same
    bits from an eager in-place execution."""
    m = batch * rows * cols
    assert tf.plan_describe(cols, 1, tf.capi.plan_default_variant(cols, 1, batch * rows)) == row_chain
    assert tf.plan_describe(rows, cols, 0) == col_chain
    rng = np.random.default_rng([23, rows, cols, batch])
    xh = rng.uniform(-1, 1, (2, m)).astype(np.float16)
    xc = xh[0].astype(np.float64) + 1j * xh[1].astype(np.float64)
    ref = (np.fft.fft2(xc.reshape(batch, rows, cols)) / (rows * cols)).reshape(batch, rows * cols)
    re, im = _dev(xh[0]), _dev(xh[1])

    def check(o_re, o_im, kernels, what):
        got = [t.cpu().numpy().astype(np.float64).reshape(batch, rows * cols) for t in (o_re, o_im)]
        worst = eb.check(got[0], got[1], ref.real, ref.imag, k_of(kernels, {"kind": "2d"}), rel_l2=eb.REL_L2, what=what)
        print(f"{what}: worst {worst:.3f} ulp")

    for own in (False, True):
        plan = tf.TfftPlan2D(rows, cols, batch, 0)
        assert plan.num_launches == len(row_chain.split()) + len(col_chain.split()), plan.kernels
        assert plan.workspace_bytes >= 2 * m * 4, "no sub-plan scratch behind the intermediate"
        o_re, o_im = torch.zeros_like(re), torch.zeros_like(im)
        what = f"2D {rows} x {cols} x {batch}, {'own' if own else 'caller'} workspace"
        if own:
            run = lambda a, b, c, d: _exec2d_c(tf, plan, a, b, c, d)          # noqa: E731
            run(re, im, o_re, o_im)                                          # eager: the library allocates here
            torch.cuda.synchronize()
            check(o_re, o_im, plan.kernels, what + ", eager")
            eager_re, eager_im = o_re.clone(), o_im.clone()
            o_re.zero_()
            o_im.zero_()
        else:
            buf, ws = _guarded_workspace(plan.workspace_bytes)
            plan.set_workspace(ws)
            run = plan.exec
        graph = _capture(lambda: run(re, im, o_re, o_im))
        _replay(graph)
        check(o_re, o_im, plan.kernels, what + ", captured")
        if own:
            assert _same(o_re, eager_re) and _same(o_im, eager_im), "captured execution differs from the eager one before it"
        else:
            assert de._guards_intact(torch, buf), "written outside the caller's workspace"
        w_re, w_im = re.clone(), im.clone()
        run(w_re, w_im, w_re, w_im)
        torch.cuda.synchronize()
        assert _same(w_re, o_re) and _same(w_im, o_im), "in place differs from out of place"
        plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. composed convolution and real-input plans: sub-plans bound to shares of one workspace
# ---------------------------------------------------------------------------------------------------------------------
def test_conv_plan_with_sub_plan_scratch(tf):
    """prepare(), first execution under capture; against the fp64 convolution, bit-identical to eager and to in place; then a
    caller's workspace of exactly workspace_bytes between guard zones: the sub-plans stay inside their share."""
    n, batch, filters, xh, ref, h_re, h_im = _conv_case()
    plan = _conv_plan(tf, n, batch, filters, h_re, h_im)
    _assert_conv_structure(plan)
    plan.prepare()
    x, y = _dev(xh), torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
    graph = _capture(lambda: plan.exec(x, x[n:], y, y[n:]))
    _replay(graph)
    _check(y, ref, batch, n, conv_ref.K_CONV_COMPOSED, "conv 2^16: captured first execution")
    assert np.array_equal(x.cpu().numpy().view(np.int16), xh.reshape(-1).view(np.int16)), "input written"
    eager = torch.zeros_like(y)
    plan.exec(x, x[n:], eager, eager[n:])
    work = x.clone()
    plan.exec(work, work[n:], work, work[n:])
    torch.cuda.synchronize()
    assert _same(eager, y), "eager differs from the captured execution"
    assert _same(work, y), "in place differs from out of place"
    plan.close()
    own = _conv_plan(tf, n, batch, filters, h_re, h_im)
    buf, ws = _guarded_workspace(own.workspace_bytes)
    own.set_workspace(ws)
    y2 = torch.zeros_like(y)
    graph2 = _capture(lambda: own.exec(x, x[n:], y2, y2[n:]))
    _replay(graph2)
    assert de._guards_intact(torch, buf), "a sub-plan wrote outside the caller's workspace"
    assert _same(y2, y), "caller's workspace: other bits than the library's own"
    own.close()


def test_real_plan_with_sub_plan_scratch(tf):
    """real-2^18 x 3: prepare(), first R2C under capture, against numpy.fft.rfft / n bin by bin and bit-identical to eager."""
    n, batch = 1 << 18, 3
    assert tf.capi.rplan_describe(n, batch) == "r2c: col:256+tw col:256+tw autosort:4-tw split | c2r: merge col:256+tw col:256+tw autosort:4-tw"
    plan = tf.TfftRealPlan(n, batch, 0)
    assert plan.num_launches(False) == 2 * 3 + 1, plan.kernels(False)     # pair + tail sub-plan, one split
    assert plan.workspace_bytes > ((batch + 1) // 2) * n * 4, "no sub-plan scratch behind the complex spectra"
    plan.prepare()
    rng = np.random.default_rng([24, n, batch])
    xh = rng.uniform(-1, 1, (batch, n)).astype(np.float16)
    h, bins = plan.pitch, n // 2 + 1
    x = _dev(xh)
    spec = torch.zeros(batch * 2 * h, dtype=torch.float16, device=DEV)
    graph = _capture(lambda: plan.r2c(x, spec, spec[h:]))
    _replay(graph)
    got = spec.cpu().numpy().astype(np.float64).reshape(batch, 2, h)
    ref = np.fft.rfft(xh.astype(np.float64), axis=1) / n
    worst = eb.check(got[:, 0, :bins], got[:, 1, :bins], ref.real, ref.imag, eb.K_REAL, rel_l2=eb.REL_L2, pairs=True, what="real 2^18 x 3: captured R2C")
    print(f"real 2^18 x 3: captured R2C: worst {worst:.3f} ulp")
    assert np.array_equal(x.cpu().numpy().view(np.int16), xh.reshape(-1).view(np.int16)), "input written"
    eager = torch.zeros_like(spec)                 # (the pitch padding is never written: the same zeros in both)
    plan.r2c(x, eager, eager[h:])
    torch.cuda.synchronize()
    assert _same(eager, spec), "eager differs from the captured execution"
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. listing a plan's kernels walks its launch logic without launching: it leaves nothing behind for the next execution
# ---------------------------------------------------------------------------------------------------------------------
def _listing_that_fails_inside_the_walk(tf):
    """auto-3 with padded batch strides and a caller's workspace of one block, asked for its in-place kernels: the chain of three
    passes would start from a copy of the [RE | IM] block, and launch_chain refuses the padded layout (TFFT_ERR_ARG) from inside the
    recording walk, behind the workspace look-up and in front of the first kernel."""
    n, batch, stride = 512, 3, 2 * 512 + 8
    plan = tf.TfftPlan(n, batch, 0, in_batch_stride=stride, out_batch_stride=stride, preserve_input=True, variant=tf.capi.VARIANT_AUTOSORT_ONLY)
    assert plan.workspace_bytes == batch * n * 4
    plan.set_workspace(torch.zeros(plan.workspace_bytes // 2, dtype=torch.float16, device=DEV))
    assert len(plan.kernels) == 3, plan.kernels                # the out-of-place walk of the same plan goes through
    # (through the C ABI itself: a listing returns its line count or a positive error code, and the binding takes a 5 for five lines)
    buf = ctypes.create_string_buffer(1 << 12)
    rc = plan._lib.tfft_plan_kernels_in_place(plan._h, buf, len(buf))
    assert rc == 5 and buf.value == b"", (rc, buf.value)                                          # TFFT_ERR_ARG, nothing listed
    assert "[RE | IM] block layout" in tf.capi.last_error(), tf.capi.last_error()                 # ... from launch_chain
    plan.close()


@pytest.mark.parametrize("sid", ["auto-3", "col-2", "tr-out", "real-4096"])
def test_listing_kernels_between_executions_changes_nothing(tf, sid):
    """Execute (against fp64), list the kernels out of place and in place, run a listing that fails inside its walk, execute again
    into a cleared buffer: the bits of the first execution, and the same listings as before."""
    if sid == "real-4096":
        n, batch = 4096, 3
        plan = tf.TfftRealPlan(n, batch, 0)
        assert plan.num_launches(False) == 1, plan.kernels(False)      # fused: the N = 4096 kernel alone
        h, bins = plan.pitch, n // 2 + 1
        rng = np.random.default_rng([26, n, batch])
        xh = rng.uniform(-1, 1, (batch, n)).astype(np.float16)
        ref = np.fft.rfft(xh.astype(np.float64), axis=1) / n
        x, y = _dev(xh), torch.zeros(batch * 2 * h, dtype=torch.float16, device=DEV)
        run = lambda out: plan.r2c(x, out, out[h:])                             # noqa: E731
        listings = lambda: (plan.kernels(False), plan.kernels(True))            # noqa: E731

        def check(out, what):
            got = out.cpu().numpy().astype(np.float64).reshape(batch, 2, h)
            worst = eb.check(got[:, 0, :bins], got[:, 1, :bins], ref.real, ref.imag, eb.K_REAL, rel_l2=eb.REL_L2, pairs=True, what=what)
            print(f"{what}: worst {worst:.3f} ulp")
    else:
        plan = make_plan(tf, sid)
        n, batch = plan.n, plan.batch
        xin, fwd, _ = _data(tf, sid)
        k = k_of(plan.kernels, {"kind": "c"})
        x, y = _dev(xin), torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
        run = lambda out: plan.exec(x, x[n:], out, out[n:])                     # noqa: E731
        listings = lambda: (plan.kernels, plan.kernels_in_place)                # noqa: E731
        check = lambda out, what: _check(out, fwd, batch, n, k, what)           # noqa: E731
    run(y)
    torch.cuda.synchronize()
    check(y, f"{sid}: first execution")
    before = listings()
    assert all(before), before
    _listing_that_fails_inside_the_walk(tf)
    again = torch.zeros_like(y)
    run(again)
    torch.cuda.synchronize()
    assert _same(again, y), "an execution after the listings differs from the one before them"
    check(again, f"{sid}: execution after the listings")
    assert listings() == before, "the listings changed"
    plan.close()


def test_listing_on_one_thread_does_not_reach_an_execution_on_another(tf):
    """The single-pass plan that test_one_plan_from_several_host_threads shares, n = 4096 x 64: one thread lists its kernels 200
    times while this one executes 20 times on a stream of its own into its own zeroed output. The bits of a quiet run, and the
    same one-line listing every time: a walk is its caller's business alone."""
    import threading

    n, batch = 4096, 64
    plan = tf.TfftPlan(n, batch, 0)
    quiet_list = plan.kernels
    assert plan.num_launches == 1 and len(quiet_list) == 1, quiet_list
    rng = np.random.default_rng([27, n, batch])
    xh = rng.uniform(-1, 1, (batch, 2, n)).astype(np.float16)
    xc = xh[:, 0].astype(np.float64) + 1j * xh[:, 1].astype(np.float64)
    x, quiet = _dev(xh), torch.zeros(batch * 2 * n, dtype=torch.float16, device=DEV)
    plan.exec(x, x[n:], quiet, quiet[n:])
    torch.cuda.synchronize()
    _check(quiet, np.fft.fft(xc, axis=1) / n, batch, n, k_of(quiet_list, {"kind": "c"}), "4096 x 64: quiet run")
    seen, errs = [], []
    started = threading.Event()

    def lister():
        try:
            for i in range(200):
                seen.append(plan.kernels)
                if i == 0:
                    started.set()
        except Exception as e:   # noqa: BLE001
            errs.append(e)
            started.set()

    got = torch.zeros_like(quiet)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = threading.Thread(target=lister)
    t.start()
    started.wait()
    for _ in range(20):
        plan.exec(x, x[n:], got, got[n:], stream.cuda_stream)
    stream.synchronize()
    t.join()
    assert not errs, errs
    assert len(seen) == 200 and all(s == quiet_list for s in seen), [s for s in seen if s != quiet_list][:3]
    assert _same(got, quiet), "an execution beside a listing thread differs from the quiet run"
    plan.close()

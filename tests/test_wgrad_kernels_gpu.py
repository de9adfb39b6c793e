"""The weight-gradient kernels of F.linear on a real MI355X, instantiation by instantiation: one launch per case of
tests/wgrad_kernel_cases.py through the C ABI against fp64 -- usf_wgrad_f32 (exact-f32, bf16x3, loader waves), usf_wgrad_bias_f32,
usf_grad_jobs_f32, usf_colsum_f32, usf_wgrad_planes_f32, usf_wgrad_blocked_f32, usf_wgrad_blocked_plan_f32 +
usf_wgrad_reduce_jobs_f32 and usf_split_planes_f32.  A NaN with a payload of its own sits wherever the launch must not read into
a result or write, the workspace is exactly the reported size, every element of G[:N, :K] and every column sum is held to
max(4 err32, 6e-8 sqrt(M)) of max |ref64|, census cases to the exact sum of the six kept products bit for bit, every other byte of
every buffer is accounted for, a second launch gives the same bits, the inputs are unchanged, and the library's own account of
what it launches (usf_wgrad_plan, usf_wgrad_planes_plan) matches the instantiation the table claims.  Nothing is tuned to the
kernels."""
import ctypes as C

import pytest
import torch

import wgrad_kernel_cases as wk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from usflows_amd import _ext
    return _ext, _ext.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_bytes(ctypes_array):
    return torch.frombuffer(bytearray(bytes(ctypes_array)), dtype=torch.uint8).to(DEV)


def _reported_plan(c, lib, ws_floats):
    """the library's account of the launch, compared field by field with the restated rules the table was built from"""
    plan = wk.case_plan(c)
    if c.entry in ("f32", "bias"):
        ldy, lda, _ = wk.case_lds(c)
        out = (C.c_int64 * 8)()
        assert lib.usf_wgrad_plan(c.M, c.N, c.K, ldy, lda, c.mode, int(c.cs), out, 8) == 8, lib.usf_last_error()
        got = dict(zip(("variant", "splits", "rows", "direct", "grid", "threads", "reduce", "need"), out))
        assert got == plan, f"usf_wgrad_plan {got} != the table's {plan}"
        assert lib.usf_wgrad_variant(c.M, c.N, c.K, ldy, lda, c.mode) == plan["variant"]
        assert plan["need"] <= ws_floats
    elif c.entry != "jobs":
        out = (C.c_int64 * 35)()
        assert lib.usf_wgrad_planes_plan(c.M, c.N, c.K, ws_floats, int(c.cs), 0, out, 35) == 35, lib.usf_last_error()
        got = dict(balanced=out[0], foldN=out[1], foldK=out[2], blocks=out[3], items=out[4], parts=out[6], T=list(out[7:16]),
                   nseg=list(out[16:25]), rows=list(out[25:34]))
        want = {k: plan[k] for k in got}
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert got == want, f"usf_wgrad_planes_plan on {cus} compute units {got} != the table's (written for {wk.CUS}) {want}"
        assert out[5] == plan["parts"] * c.N * (c.K + int(c.cs)) <= ws_floats


def _launch(c, p, job=None):
    """ONE launch (plan entry: the multiply launch alone, `job` filled) on device copies of the case's buffers"""
    ext, lib = _lib()
    Y, A = p["Y"].to(DEV), p["A"].to(DEV)
    G, cs, ws = p["G0"].to(DEV), p["cs0"].to(DEV), p["ws0"].to(DEV)
    ldy, lda, ldg = wk.case_lds(c)
    M, N, K = c.M, c.N, c.K
    gp, csp = G.data_ptr() + 4 * wk.GF, (cs.data_ptr() + 4 * wk.GF) if c.cs else None
    keep = [Y, A, G, cs, ws]
    with wk.knobs(c.kn):
        if c.entry in ("f32", "bias"):
            wsf = lib.usf_wgrad_workspace_floats(M, N, K)
            assert wsf == wk.case_workspace_floats(c) == ws.numel() - wk.GF
            _reported_plan(c, lib, wsf)
            yp, ap = Y.data_ptr() + 4 * wk.GF, A.data_ptr() + 4 * wk.GF
            if c.entry == "bias":
                assert lib.usf_wgrad_bias_ok(M, N, K, ldy, lda, c.mode) == 1
                rc = lib.usf_wgrad_bias_f32(yp, ldy, ap, lda, M, N, K, gp, ldg, c.alpha, c.beta, c.mode, csp, *c.cs_ab, ws.data_ptr(), wsf,
                                            _stream())
            else:
                rc = lib.usf_wgrad_f32(yp, ldy, ap, lda, M, N, K, gp, ldg, c.alpha, c.beta, c.mode, ws.data_ptr(), wsf, _stream())
        elif c.entry == "jobs":
            jb = (ext.GradJob * 1)()
            jb[0].Y, jb[0].A, jb[0].G = Y.data_ptr() + 4 * wk.GF, A.data_ptr() + 4 * wk.GF, gp
            jb[0].ldy, jb[0].lda, jb[0].ldg, jb[0].M, jb[0].N, jb[0].K = ldy, lda, ldg, M, N, K
            jb[0].first_block, jb[0].alpha, jb[0].beta = 0, c.alpha, c.beta
            nb = wk.wg_tiles(N, K)
            jobs, bj = _dev_bytes(jb), torch.zeros(nb, dtype=torch.int32, device=DEV)
            keep += [jobs, bj]
            rc = lib.usf_grad_jobs_f32(jobs.data_ptr(), bj.data_ptr(), nb, _stream())
        else:
            wsf = lib.usf_wgrad_planes_workspace_floats(M, N, K)
            assert wsf == wk.case_workspace_floats(c) == ws.numel() - wk.GF, \
                f"the workspace on this device ({wsf}) is not the table's ({wk.case_workspace_floats(c)}, written for {wk.CUS} compute units)"
            _reported_plan(c, lib, wsf)
            assert not c.cs or lib.usf_wgrad_planes_colsum_ok(M, N, K) == 1
            yp, ap = Y.data_ptr() + 2 * wk.GH, A.data_ptr() + 2 * wk.GH
            tail = (M, N, K, gp, ldg, c.alpha, c.beta, csp, *c.cs_ab, ws.data_ptr(), wsf)
            if c.entry == "planes":
                rc = lib.usf_wgrad_planes_f32(yp, ldy, p["ystride"], c.off[0], ap, lda, p["astride"], c.off[1], *tail, _stream())
            else:
                y_nkb, a_nkb = wk.case_nkb(c)
                head = (yp, y_nkb, c.off[0], ap, a_nkb, c.off[1])
                if c.entry == "plan":
                    rc = lib.usf_wgrad_blocked_plan_f32(*head, *tail, C.byref(job), _stream())
                else:
                    rc = lib.usf_wgrad_blocked_f32(*head, *tail, _stream())
    assert rc == 0, lib.usf_last_error()
    if c.entry == "plan":
        return dict(G=G, cs=cs, ws=ws, keep=keep, inputs=(Y, A))
    torch.cuda.synchronize()
    for name, t in (("Y", Y), ("A", A)):
        assert torch.equal(t.cpu().view(torch.uint8), p[name].view(torch.uint8)), f"the launch changed its input {name}"
    return dict(G=G.cpu(), cs=cs.cpu(), ws=ws.cpu())


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("G", "cs"))


def _live(c, got, p):
    return wk.g_view(c, got["G"], p["ldg"])[:c.N, :c.K].contiguous().view(torch.int32)


def _twin(c, **kw):
    return c._replace(**kw)


@pytest.mark.parametrize("c", wk.F32_CASES + wk.PLANES_CASES, ids=wk.case_id)
def test_wgrad_kernel_vs_fp64(c):
    p = wk.prepared(c)
    got = _launch(c, p)
    bad, fig = wk.check(c, got, p)
    print(wk.report_line(c, fig))
    assert bad == []
    assert _same(_launch(c, p), got), "a second launch gives other bits"
    # the equivalences the headers state, bit for bit
    if c.entry == "jobs":
        t = _twin(c, entry="f32")
        assert torch.equal(_live(t, _launch(t, wk.prepared(t)), wk.prepared(t)), _live(c, got, p)), \
            "usf_grad_jobs_f32 is not usf_wgrad_f32 mode 0 at M <= 256"
    if c.entry == "bias":
        t = _twin(c, entry="f32", cs=False, cs_ab=(0.0, 0.0))
        assert torch.equal(_live(t, _launch(t, wk.prepared(t)), wk.prepared(t)), _live(c, got, p)), \
            "usf_wgrad_bias_f32's G is not usf_wgrad_f32's"
    if c.entry == "blocked" and c.idx % 2 == 0:
        t = _twin(c, entry="planes", off=(8 * c.off[0], 8 * c.off[1]), pad=(8, 16, c.pad[2]))
        assert wk.case_plan(t) == wk.case_plan(c)
        tg = _launch(t, wk.prepared(t))
        assert torch.equal(_live(t, tg, wk.prepared(t)), _live(c, got, p)), "blocked operands give other bits than row-major planes"
        if c.cs:
            assert torch.equal(tg["cs"].view(torch.int32), got["cs"].view(torch.int32))


# the smallest shape the loader-wave kernel takes (20 full tiles at 8192 rows), and one with edge tiles
LW_EQUIV = [wk._w("planes", "table", 1, 8192, 640, 512, 5000, ab=(1.0, 0.0), kn=(("wgrad_sched", 0),)),
            wk._w("planes", "table", 1, 8193, 528, 448, 5001, ab=(1.0, 0.0), kn=(("wgrad_sched", 0),))]


@pytest.mark.parametrize("c", LW_EQUIV, ids=wk.case_id)
def test_planes_on_the_plain_grid_equal_the_loader_wave_kernel(c):
    p = wk.prepared(c)
    assert wk.case_plan(c)["balanced"] == 0
    got = _launch(c, p)
    bad, fig = wk.check(c, got, p)
    print(wk.report_line(c, fig))
    assert bad == []
    t = wk._w("f32", "table", 1, c.M, c.N, c.K, c.idx, ab=(1.0, 0.0))
    tp = wk.prepared(t)
    assert wk.case_plan(t)["variant"] == 2 and torch.equal(tp["Yv"], p["Yv"]) and torch.equal(tp["Av"], p["Av"])
    tg = _launch(t, tp)
    assert wk.check(t, tg, tp)[0] == []
    assert torch.equal(_live(t, tg, tp), _live(c, got, p)), "usf_wgrad_planes_f32 on the plain grid is not the loader-wave kernel"


def test_three_gradients_reduced_in_one_jobs_launch_equal_the_undeferred_calls():
    ext, lib = _lib()
    jobs = (ext.WReduceJob * len(wk.PLAN_CASES))()
    runs, first = [], 0
    for i, c in enumerate(wk.PLAN_CASES):
        p = wk.prepared(c)
        runs.append((c, p, _launch(c, p, jobs[i])))
        assert jobs[i].blocks > 0
        jobs[i].first_block = first
        first += jobs[i].blocks
    bj = torch.cat([torch.full((jobs[i].blocks,), i, dtype=torch.int32) for i in range(len(wk.PLAN_CASES))]).to(DEV)
    torch.cuda.synchronize()
    for c, p, r in runs:          # the plan call leaves G and colsum_out unwritten
        assert torch.equal(r["G"].cpu().view(torch.int32), p["G0"].view(torch.int32))
        assert torch.equal(r["cs"].cpu().view(torch.int32), p["cs0"].view(torch.int32))
    dj = _dev_bytes(jobs)
    assert lib.usf_wgrad_reduce_jobs_f32(dj.data_ptr(), bj.data_ptr(), first, _stream()) == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    for c, p, r in runs:
        got = dict(G=r["G"].cpu(), cs=r["cs"].cpu(), ws=r["ws"].cpu())
        for name, t in zip(("Y", "A"), r["inputs"]):
            assert torch.equal(t.cpu().view(torch.uint8), p[name].view(torch.uint8)), f"the launch changed its input {name}"
        bad, fig = wk.check(c, got, p)
        print(wk.report_line(c, fig))
        assert bad == []
        t = _twin(c, entry="blocked")
        assert _same(_launch(t, wk.prepared(t)), got), "plan + usf_wgrad_reduce_jobs_f32 is not usf_wgrad_blocked_f32"


def _colsum_launch(c, p):
    ext, lib = _lib()
    Y, out, ws = p["Y"].to(DEV), p["out0"].to(DEV), p["ws0"].to(DEV)
    yp, op = Y.data_ptr() + 4 * wk.GF, out.data_ptr() + 4 * wk.GF
    if c.entry == "colsum":
        rc = lib.usf_colsum_f32(yp, p["ld"], c.M, c.N, op, c.alpha, c.beta, ws.data_ptr(), ws.numel() - wk.GF, _stream())
    else:
        jb = (ext.GradJob * 1)()
        jb[0].Y, jb[0].A, jb[0].G, jb[0].ldy, jb[0].M, jb[0].N = yp, None, op, p["ld"], c.M, c.N
        jb[0].first_block, jb[0].alpha, jb[0].beta = 0, c.alpha, c.beta
        nb = wk.cdiv(c.N, 64)
        jobs, bj = _dev_bytes(jb), torch.zeros(nb, dtype=torch.int32, device=DEV)
        rc = lib.usf_grad_jobs_f32(jobs.data_ptr(), bj.data_ptr(), nb, _stream())
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(Y.cpu().view(torch.int32), p["Y"].view(torch.int32)), "the launch changed its input"
    return dict(out=out.cpu(), ws=ws.cpu())


@pytest.mark.parametrize("c", wk.COLSUM_CASES, ids=wk.ccase_id)
def test_colsum_kernels_vs_fp64(c):
    p = wk.colsum_prepared(c)
    got = _colsum_launch(c, p)
    bad, fig = wk.colsum_check(c, got, p)
    print(f"WK|{c.entry}|levels{wk.colsum_levels(c.M) if c.entry == 'colsum' else 1}|{c.kind}|M{c.M} N{c.N}|{fig['err']:.3e}|{fig['err32']:.3e}"
          f"|{fig['bound']:.3e}||{fig['census']}")
    assert bad == []
    assert torch.equal(_colsum_launch(c, p)["out"].view(torch.int32), got["out"].view(torch.int32)), "a second launch gives other bits"


def test_grad_jobs_of_both_kinds_in_one_launch_with_block_offsets():
    """every weight job and every column-sum job of the tables queued in ONE usf_grad_jobs_f32 launch (first_block > 0 for all
    but the first): each job's result passes its own check and has the bits of its single launch"""
    ext, lib = _lib()
    wjobs = [c for c in wk.F32_CASES if c.entry == "jobs"]
    cjobs = [c for c in wk.COLSUM_CASES if c.entry == "jobcs"]
    order = [x for pair in zip(wjobs, cjobs) for x in pair] + cjobs[len(wjobs):] + wjobs[len(cjobs):]
    jb = (ext.GradJob * len(order))()
    bufs, block_job, first = [], [], 0
    for i, c in enumerate(order):
        if c.entry == "jobs":
            p = wk.prepared(c)
            ldy, lda, ldg = wk.case_lds(c)
            d = dict(Y=p["Y"].to(DEV), A=p["A"].to(DEV), G=p["G0"].to(DEV))
            jb[i].Y, jb[i].A, jb[i].G = d["Y"].data_ptr() + 4 * wk.GF, d["A"].data_ptr() + 4 * wk.GF, d["G"].data_ptr() + 4 * wk.GF
            jb[i].ldy, jb[i].lda, jb[i].ldg, jb[i].M, jb[i].N, jb[i].K = ldy, lda, ldg, c.M, c.N, c.K
            nb = wk.wg_tiles(c.N, c.K)
        else:
            p = wk.colsum_prepared(c)
            d = dict(Y=p["Y"].to(DEV), G=p["out0"].to(DEV))
            jb[i].Y, jb[i].A, jb[i].G = d["Y"].data_ptr() + 4 * wk.GF, None, d["G"].data_ptr() + 4 * wk.GF
            jb[i].ldy, jb[i].M, jb[i].N = p["ld"], c.M, c.N
            nb = wk.cdiv(c.N, 64)
        jb[i].first_block, jb[i].alpha, jb[i].beta = first, c.alpha, c.beta
        block_job += [i] * nb
        first += nb
        bufs.append((c, p, d))
    jobs, bj = _dev_bytes(jb), torch.tensor(block_job, dtype=torch.int32).to(DEV)
    assert lib.usf_grad_jobs_f32(jobs.data_ptr(), bj.data_ptr(), first, _stream()) == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    for c, p, d in bufs:
        assert torch.equal(d["Y"].cpu().view(torch.int32), p["Y"].view(torch.int32))
        if c.entry == "jobs":
            got = dict(G=d["G"].cpu(), cs=p["cs0"], ws=p["ws0"])
            assert wk.check(c, got, p)[0] == [], wk.case_id(c)
            assert torch.equal(got["G"].view(torch.int32), _launch(c, p)["G"].view(torch.int32)), wk.case_id(c)
        else:
            got = dict(out=d["G"].cpu(), ws=p["ws0"])
            assert wk.colsum_check(c, got, p)[0] == [], wk.ccase_id(c)
            assert torch.equal(got["out"].view(torch.int32), _colsum_launch(c, p)["out"].view(torch.int32)), wk.ccase_id(c)


def _split_launch(c, p):
    _, lib = _lib()
    X, P = p["X"].to(DEV), p["P0"].to(DEV)
    xp = X.data_ptr() + 4 * p["x_off"]
    assert (xp % 16 == 0) == (c.path != "misaligned")
    rc = lib.usf_split_planes_f32(xp, c.ldx, c.M, c.N, P.data_ptr() + 2 * wk.GH, c.ldp, p["stride"], _stream())
    assert rc == 0, lib.usf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(X.cpu().view(torch.int32), p["X"].view(torch.int32)), "the launch changed its input"
    return P.cpu()


@pytest.mark.parametrize("c", wk.SPLIT_CASES, ids=wk.scase_id)
def test_split_planes_kernel_bit_for_bit(c):
    p = wk.split_prepared(c)
    got = _split_launch(c, p)
    if c.path.startswith("sweep"):
        R, st = wk.ceil_to(c.M, 32), p["stride"]
        planes = torch.stack([got[wk.GH + q * st: wk.GH + q * st + R * c.ldp].view(R, c.ldp)[:c.M, :c.N] for q in range(3)])
        rng = wk.split_exact_exponents(wk.split_exact_rows(planes, p["Xv"]))
        print(f"WK|split|{'vector' if wk.split_is_vector(c) else 'scalar'}|sweep|p0 + p1 + p2 == x bit for bit for 2^{rng[0]} <= |x| < 2^{rng[1] + 1}")
        assert rng == (wk.SPLIT_EXACT_EMIN, wk.SPLIT_EXACT_EMAX)
    assert wk.split_check(c, got, p) == []
    assert torch.equal(_split_launch(c, p), got), "a second launch gives other bits"
    assert torch.equal(got[:wk.GH], p["P0"][:wk.GH]) and torch.equal(got[-wk.GH:], p["P0"][-wk.GH:])

"""Every row of tests/conv_wgrad_band_cases.py, in every form, launched on the device and held to the fp64 statement on EVERY
element: |got - fp64| <= MARGIN * K * U * A and the suite's max-norm bound, sentinels in front of and behind every output, one
NaN sample behind x and dy, a workspace full of NaN, the same bits from a second launch.  Beside them: the plan's band against a
capped one, the wide kernel on a map both serve, and refusals that write nothing.  The reference runs in fp64 on the device (the
torch statements tests/test_conv_wgrad_band_cpu.py holds the fp32 statements to).

Measured (MI355X): the worst share of the per-element bound over the table is printed per case as ``WGB``; the figures are
recorded in profiles/conv_wgrad_band_parity.md."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_wgrad_band_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ext():
    from usflows_amd import _ext
    return _ext


def _rows_nan(t):
    """[B, ...] -> (buffer kept alive, view of the B samples); one NaN sample lies behind them"""
    flat = torch.full((t.numel() + t[0].numel(),), float("nan"), dtype=torch.float32, device=DEV)
    flat[:t.numel()] = t.flatten().to(DEV)
    return flat, flat[:t.numel()].view(t.shape)


class Launch:
    """one case's operands on the device; ``run`` launches into fresh guarded buffers and a workspace full of NaN"""

    def __init__(self, c):
        self.c = c
        d = G.wg_data(c)
        self.kx, self.x = _rows_nan(d.x)
        self.ky, self.dy = _rows_nan(d.dy)
        self.in_mul = None if d.in_mul is None else d.in_mul.to(DEV)
        self.pre_sub = None if d.pre_sub is None else d.pre_sub.to(DEV)

    def on_device(self):
        return G.Case(x=self.x, dy=self.dy, in_mul=self.in_mul, pre_sub=self.pre_sub)

    def run(self, band_rows=None, short_ws=False):
        c, ext = self.c, _ext()
        lib = ext.load()
        rb = c.band_rows if band_rows is None else band_rows
        p = lambda t: None if t is None else t.data_ptr()
        bufW, bufb = G.guarded(c.cout * c.cin * c.ks * c.ks, DEV), G.guarded(c.cout, DEV)
        with G.block_cap(lib, c.cap):
            ws_n = lib.usf_conv_wgrad_band_workspace(c.B, c.cin, c.cout, c.H, c.W, c.ks, rb)
            ws = torch.full((max(ws_n, 16),), float("nan"), dtype=torch.float32, device=DEV)
            rc = lib.usf_conv_wgrad_band_f32(self.x.data_ptr(), self.dy.data_ptr(), c.B, c.cin, c.cout, c.H, c.W, c.ks, p(self.in_mul),
                                             p(self.pre_sub), c.act, c.slope, bufW.data_ptr() + 4 * G.GUARD,
                                             bufb.data_ptr() + 4 * G.GUARD if c.bias else None, ws.data_ptr(),
                                             ws_n - 1 if short_ws else ws_n, rb, ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, bufW, bufb


def _hold(c, L, r, rc, bufW, bufb, tag=""):
    assert rc == 0, (c.name, rc, _ext().load().usf_last_error())
    found = G.check("dW", bufW, r.dW, r.A_dW, "dW")
    line = f"WGB {c.name}{tag} dW {G.ratio(bufW[G.GUARD:G.GUARD + r.dW.numel()].view(r.dW.shape), r.dW, r.A_dW) / (G.MARGIN * G.K['dW']):.4f} of the bound, " \
           f"max-norm {G.maxnorm(bufW[G.GUARD:G.GUARD + r.dW.numel()].view(r.dW.shape), r.dW):.3e}"
    if c.bias:
        found += G.check("db", bufb, r.db, r.A_db, "db")
        line += f"; db {G.ratio(bufb[G.GUARD:G.GUARD + c.cout], r.db, r.A_db) / (G.MARGIN * G.K['db']):.4f} of the bound, " \
                f"max-norm {G.maxnorm(bufb[G.GUARD:G.GUARD + c.cout], r.db):.3e}"
    else:
        assert G.untouched(bufb), f"{c.name}: db == NULL, yet the buffer next to dW was written"
    print(line)
    assert found == [], (c.name + tag, found)


@pytest.mark.parametrize("row", G.ROWS, ids=G.name_of)
def test_every_row_form_and_element_against_fp64(row):
    ext = _ext()
    for form in G.FORMS:
        c = G.case(row, form)
        with G.block_cap(ext.load(), c.cap):
            v = ext.conv_wgrad_band_variant(c.B, c.cin, c.cout, c.H, c.W, c.ks, band_rows=c.band_rows)
        assert v["served"] == 1, c.name
        L = Launch(c)
        rc, bufW, bufb = L.run()
        r = G.wg_forward(c, L.on_device(), torch.float64)
        _hold(c, L, r, rc, bufW, bufb)
        rc2, bufW2, bufb2 = L.run()
        assert rc2 == 0 and torch.equal(G.bits(bufW2), G.bits(bufW)) and torch.equal(G.bits(bufb2), G.bits(bufb)), \
            f"{c.name}: a second launch gives other bits"
        if form in ("mask_relu", "presub_leaky"):
            # the plan's band against a capped one (in_mul and pre_sub at the absolute pixel under another banding): other sums in
            # another order, both inside the bound (not bit-equal)
            other = 3 if v["band_rows"] != 3 else 2
            rc3, bufW3, bufb3 = L.run(band_rows=other)
            _hold(c, L, r, rc3, bufW3, bufb3, tag=f" [band_rows={other}]")


def test_every_instantiation_is_launched_by_the_table():
    ext = _ext()
    launched = set()
    for row in G.ROWS:
        c = G.case(row, "plain")
        launched.add(ext.conv_wgrad_band_variant(c.B, c.cin, c.cout, c.H, c.W, c.ks, band_rows=c.band_rows)["tiles_per_wave"])
    assert sorted(launched) == sorted(ext.conv_wgrad_band_instances())


def test_a_16x16_map_agrees_with_the_wide_kernel():
    cin, cout, H, W, ks, B = G.SMALL_MAP
    ext = _ext()
    for form in ("mask_relu", "presub_leaky"):
        c = G.case((cin, cout, H, W, ks, 0, B, 0), form)
        L = Launch(c)
        r = G.wg_forward(c, L.on_device(), torch.float64)
        rc, bufW, bufb = L.run()
        _hold(c, L, r, rc, bufW, bufb)
        wide = ext.conv_wgrad_wide(L.x, L.dy, ks, in_mul=L.in_mul, pre_sub=L.pre_sub, in_act=c.act, in_slope=c.slope)
        assert wide is not None
        # the two kernels within the bound of EACH OTHER, element by element, and the wide kernel's result within it of fp64 too
        dW = bufW[G.GUARD:G.GUARD + r.dW.numel()].view(r.dW.shape)
        db = bufb[G.GUARD:G.GUARD + cout]
        for got, other, ref, A, fam in ((dW, wide[0], r.dW, r.A_dW, "dW"), (db, wide[1], r.db, r.A_db, "db")):
            bound = G.MARGIN * G.K[fam] * G.U * A
            print(f"WGB-WIDE {c.name} {fam}: band - wide {G.ratio(got, other.double(), A):.3f} U A, wide - fp64 {G.ratio(other, ref, A):.3f} U A "
                  f"(bound {G.MARGIN * G.K[fam]:.2f})")
            assert bool(((got.double() - other.double()).abs() <= bound).all()), fam
            assert bool(((other.double() - ref).abs() <= bound).all()), fam


def test_refusals_write_nothing():
    ext = _ext()
    lib = ext.load()
    for cin, cout, H, W, ks in G.REFUSED:
        c = G.case((cin, cout, H, W, ks, 0, 2, 0), "plain")
        assert lib.usf_conv_wgrad_band_workspace(c.B, cin, cout, H, W, ks, 0) == 0
        assert ext.conv_wgrad_band_variant(c.B, cin, cout, H, W, ks)["served"] == 0
        x = torch.randn(c.B, cin, H, W, device=DEV)
        dy = torch.randn(c.B, cout, H, W, device=DEV)
        bufW, bufb, ws = G.guarded(cout * cin * ks * ks, DEV), G.guarded(cout, DEV), G.guarded(1 << 16, DEV)
        rc = lib.usf_conv_wgrad_band_f32(x.data_ptr(), dy.data_ptr(), c.B, cin, cout, H, W, ks, None, None, 0, 0.0,
                                         bufW.data_ptr() + 4 * G.GUARD, bufb.data_ptr() + 4 * G.GUARD, ws.data_ptr() + 4 * G.GUARD, 1 << 16, 0,
                                         ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        assert rc == 1 and G.untouched(bufW) and G.untouched(bufb) and G.untouched(ws), (cin, cout, H, W, ks)
        assert ext.conv_wgrad_band(x, dy, ks) is None
    # a workspace one float short and an empty batch: errors, nothing launched
    c = G.case(G.ROWS[0], "plain")
    L = Launch(c)
    rc, bufW, bufb = L.run(short_ws=True)
    assert rc < 0 and b"workspace too small" in lib.usf_last_error() and G.untouched(bufW) and G.untouched(bufb)
    assert lib.usf_conv_wgrad_band_f32(L.x.data_ptr(), L.dy.data_ptr(), 0, c.cin, c.cout, c.H, c.W, c.ks, None, None, 0, 0.0,
                                       bufW.data_ptr() + 4 * G.GUARD, None, bufb.data_ptr(), 16, 0, ext.current_stream(torch.device(DEV))) == -2
    torch.cuda.synchronize()
    assert G.untouched(bufW) and G.untouched(bufb)
    assert C.sizeof(ext.ConvWgradBandQuery) == lib.usf_sizeof_desc(29) and C.sizeof(ext.ConvWgradBandInfo) == lib.usf_sizeof_desc(30)

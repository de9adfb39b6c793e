"""The two MFMA families of usf_coupling_additive_f32 -- the exact-f32 kernel (usf_coupling.hip: NH in {1, 2, 3} x padded width
Hp in {64, 128, 256}) and the bf16x3 kernel (usf_coupling_bf16x3.hip: NH in {1, 2, 3}, plain / context / hidden_out / gate) --
one launch at a time against fp64: the case table, a descriptor builder that knows nothing but the header's padding contract
(include/usflows_hip.h, "Padding contract" and the split-plane fields of usf_coupling_desc: no engine packer is involved), the
fp64 / fp32 formulation of the layer (tests/test_kernels_gpu.py::test_tiny_layer_coupling_kernel states it) and the checker.
Importable without a GPU: tests/test_coupling_kernels_cpu.py holds the table and the checker to account, and
tests/test_coupling_kernels_gpu.py launches."""
import collections
import contextlib
import ctypes
import functools

import torch

ACT_NONE, ACT_LEAKY_RELU, ACT_GATE = 0, 1, 2          # include/usflows_hip.h: USF_ACT_*
VARIANT = {"f32": 1, "bf16x3": 2}                     # usf_coupling_variant (include/usflows_hip_internal.h)
EXTRA_ROWS = 3                                        # rows below M in every row buffer: NaN in z / context / gate, sentinel in hidden_out
SENTINEL = 9.0                                        # what hidden_out buffers start as
HIDDEN_SLACK, GATE_SLACK = 8, 4                       # columns of hidden_out / gate buffers beyond the padded width

Case = collections.namedtuple("Case", "family M off_pass n_pass off_trans n_trans ldz hidden act slope sign mode")


def ceil_to(n, m):
    return (n + m - 1) // m * m


def padded_width(h):
    """usf_coupling_padded_width"""
    return 64 if h <= 64 else (128 if h <= 128 else 256)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
def _layout(order, n_pass, n_trans, lead, mid, tail):
    """(off_pass, off_trans, ldz): the two segments in either order with `lead` slack columns in front, `mid` between and `tail`
    behind them (multiples of 4; the columns [n_trans, ceil4(n_trans)) are slack too)"""
    nt4 = ceil_to(n_trans, 4)
    if order == "pt":
        off_pass = lead
        off_trans = off_pass + n_pass + mid
        return off_pass, off_trans, off_trans + nt4 + tail
    off_trans = lead
    off_pass = off_trans + nt4 + mid
    return off_pass, off_trans, off_pass + n_pass + tail


_ACTS = [(ACT_LEAKY_RELU, 0.01), (ACT_LEAKY_RELU, 0.0), (ACT_NONE, 0.0)]          # leaky 0.01, ReLU, no activation

F32_WIDTHS = [(64,), (1,), (100,), (129,),                                        # NH 1: Hp 64, 64, 128, 256
              (40, 24), (65, 128), (128, 7), (200, 136),                          # NH 2: Hp 64, 128, 128, 256
              (7, 64, 33), (65, 1, 128), (7, 130, 256), (256, 256, 256)]          # NH 3: Hp 64, 128, 256, 256
F32_M = [1, 15, 16, 17, 63, 64, 65, 257, 300]
N_PASS = [4, 16, 20, 32, 36, 52, 100]
N_TRANS = [1, 3, 4, 30, 32, 33, 37, 65]
F32_PER_WIDTHS = 4

B3_WIDTHS = [(129,), (256,), (200, 256), (256, 160), (136, 256, 130)]
B3_M = [1024, 1025, 1151, 1153]
B3_MODES = ["plain", "ctx", "hidden_out", "gate"]
# (n_pass, n_trans): one or two 16-k steps, full or masked, one or more slabs; partial float4 stores and the n-tile boundary
B3_SEGMENTS = [(4, 1), (16, 3), (20, 4), (32, 30), (36, 32), (52, 33), (100, 37), (16, 65)]


def _build_cases():
    cases = []
    # exact-f32 kernel: every (NH, Hp) instantiation at four shapes; M, n_pass and n_trans cycle through their lists with
    # pairwise coprime periods (9, 7, 8), so every value meets many others
    for w, hidden in enumerate(F32_WIDTHS):
        for j in range(F32_PER_WIDTHS):
            i = w * F32_PER_WIDTHS + j
            M, n_pass, n_trans = F32_M[i % 9], N_PASS[i % 7], N_TRANS[i % 8]
            act, slope = _ACTS[i % 3]
            off_pass, off_trans, ldz = _layout("pt" if i % 2 == 0 else "tp", n_pass, n_trans, 4 * (i % 2), 4 + 4 * (i % 3 == 0), 4 + 8 * (i % 4 == 1))
            mode = "ctx" if (i // 2) % 2 == 1 else "plain"
            cases.append(Case("f32", M, off_pass, n_pass, off_trans, n_trans, ldz, hidden, act, slope, 1.0 if (i // 3) % 2 == 0 else -1.0, mode))
    # bf16x3 kernel: all four modes of every width set; the segment edges cycle with period 8 against 4 modes x 5 width sets
    i = 0
    for w, hidden in enumerate(B3_WIDTHS):
        for mode in B3_MODES:
            for rep in range(2):
                M = B3_M[(i + w) % 4]
                n_pass, n_trans = B3_SEGMENTS[(3 * i + w) % 8]
                act, slope = _ACTS[i % 3]
                if mode == "gate":
                    act, slope = ACT_GATE, (0.01, 0.0)[rep]
                off_pass, off_trans, ldz = _layout("pt" if (i // 2 + rep) % 2 == 0 else "tp", n_pass, n_trans, 4 * (i % 2), 4 + 4 * (i % 3 == 0), 4 + 8 * (i % 4 == 1))
                cases.append(Case("bf16x3", M, off_pass, n_pass, off_trans, n_trans, ldz, hidden, act, slope, 1.0 if (i // 4 + rep) % 2 == 0 else -1.0, mode))
                i += 1
    return cases


CASES = _build_cases()


def case_id(c):
    return (f"{c.family}-M{c.M}-p{c.n_pass}at{c.off_pass}-t{c.n_trans}at{c.off_trans}-ld{c.ldz}-h{'x'.join(map(str, c.hidden))}"
            f"-{('none', 'leaky', 'gate')[c.act]}{c.slope}-{'fwd' if c.sign > 0 else 'bwd'}-{c.mode}")


def instantiation(c):
    """(family, NH, Hp): the kernel instantiation a case runs"""
    return c.family, len(c.hidden), padded_width(max(c.hidden))


# ---- weights, inputs, the layer in fp64 / fp32 ------------------------------------------------------------------------------------
def _seed(*ints):
    s = 12345
    for v in ints:
        s = (s * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def weights(n_pass, hidden, n_trans):
    """one weight set per distinct (n_pass, hidden, n_trans): Ws[l] [dims[l + 1], dims[l]] = randn / sqrt(fan_in), bs[l] = 0.1 randn,
    and the context branch's Wc, bc [hidden[0]] = randn (the distributions of test_tiny_layer_coupling_kernel)"""
    g = torch.Generator().manual_seed(_seed(n_pass, n_trans, *hidden))
    dims = [n_pass] + list(hidden) + [n_trans]
    Ws = [torch.randn(dims[l + 1], dims[l], generator=g) / dims[l] ** 0.5 for l in range(len(dims) - 1)]
    bs = [torch.randn(dims[l + 1], generator=g) * 0.1 for l in range(len(dims) - 1)]
    Wc, bc = torch.randn(hidden[0], generator=g), torch.randn(hidden[0], generator=g)
    return dict(Ws=Ws, bs=bs, Wc=Wc, bc=bc)


def _nan_like(rows, cols):
    """quiet NaNs with a payload of their own each: a NaN that moved is a different NaN"""
    lin = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    return (0x7FC00000 + 1 + lin % 0x3FFFFE).to(torch.int32).view(torch.float32)


def segment_masks(c):
    """boolean [M + EXTRA_ROWS, ldz] masks: the conditioning segment and the transformed segment of the rows [0, M)"""
    rows = c.M + EXTRA_ROWS
    p, t = torch.zeros(rows, c.ldz, dtype=torch.bool), torch.zeros(rows, c.ldz, dtype=torch.bool)
    p[: c.M, c.off_pass: c.off_pass + c.n_pass] = True
    t[: c.M, c.off_trans: c.off_trans + c.n_trans] = True
    return p, t


def forward(c, z, w, ctx, gates, dtype, drop_last_kstep=False, hidden_bias=None):
    """the layer in `dtype` on the rows z [M, ldz]: (transformed columns of the result [M, n_trans], activations of every hidden
    layer).  Gate mode: v * (gate > 0 ? 1 : slope) in place of the activation.  drop_last_kstep: W_in without its last 16-k step
    (a defect for the checker's own test)"""
    nh = len(c.hidden)
    Ws = [W.to(dtype) for W in w["Ws"]]
    bs = [b.to(dtype) for b in w["bs"]]
    if drop_last_kstep:
        Ws[0] = Ws[0].clone()
        Ws[0][:, (c.n_pass - 1) // 16 * 16:] = 0
    h = z[:, c.off_pass: c.off_pass + c.n_pass].to(dtype)
    hs = []
    for l in range(nh):
        v = h @ Ws[l].t() + bs[l]
        if c.mode == "gate":
            v = v * torch.where(gates[l][:, : c.hidden[l]].to(dtype) > 0, 1.0, c.slope).to(dtype)
        else:
            if l == 0 and c.mode == "ctx":
                v = v + (ctx.to(dtype)[:, None] * w["Wc"].to(dtype)[None, :] + w["bc"].to(dtype)[None, :])
            if c.act == ACT_LEAKY_RELU:
                v = torch.where(v > 0, v, v * c.slope)
        hs.append(v)
        h = v
    t = h @ Ws[nh].t() + bs[nh]
    return z[:, c.off_trans: c.off_trans + c.n_trans].to(dtype) + c.sign * t, hs


def _bound(ref64, ref32):
    """(err32, bound): max(4 err32, 2e-6 max(1, max |ref|)) -- the rule of test_linear_parity with the floor of
    test_tiny_layer_coupling_kernel; err32 = the error of the fp32 torch-CPU evaluation of the same values"""
    err32 = (ref32.double() - ref64).abs().max().item()
    return err32, max(4 * err32, 2e-6 * max(1.0, ref64.abs().max().item()))


@functools.lru_cache(maxsize=None)
def prepared(c):
    """inputs and references of a case, built once: z [M + EXTRA_ROWS, ldz] with randn in the two segments of the rows [0, M)
    and NaN everywhere else, context / gates likewise, the fp64 and fp32 results with their bounds"""
    g = torch.Generator().manual_seed(_seed(c.M, c.ldz, c.off_pass, c.n_pass, c.off_trans, c.n_trans, c.act, len(c.mode), *c.hidden))
    rows, nh = c.M + EXTRA_ROWS, len(c.hidden)
    Hp = padded_width(max(c.hidden))
    pmask, tmask = segment_masks(c)
    z = torch.where(pmask | tmask, torch.randn(rows, c.ldz, generator=g), _nan_like(rows, c.ldz))
    assert torch.equal(torch.isnan(z), ~(pmask | tmask))
    ctx = gates = None
    if c.mode == "ctx":
        ctx = _nan_like(rows, 1)[:, 0].contiguous()
        ctx[: c.M] = torch.randn(c.M, generator=g)
    if c.mode == "gate":
        # what the forward's hidden_out holds (zeros in the padded units' columns), NaN beyond the padded width and below M
        gates = []
        for l in range(nh):
            gt = _nan_like(rows, Hp + GATE_SLACK)
            gt[: c.M, :Hp] = 0.0
            gt[: c.M, : c.hidden[l]] = torch.randn(c.M, c.hidden[l], generator=g)
            gates.append(gt)
    w = weights(c.n_pass, c.hidden, c.n_trans)
    zl = z[: c.M]
    cl, gl = (None if ctx is None else ctx[: c.M]), (None if gates is None else [gt[: c.M] for gt in gates])
    ref64, hs64 = forward(c, zl, w, cl, gl, torch.float64)
    ref32, hs32 = forward(c, zl, w, cl, gl, torch.float32)
    err32, bound = _bound(ref64, ref32)
    return dict(z=z, ctx=ctx, gates=gates, w=w, ref64=ref64, ref32=ref32, hs64=hs64, hs32=hs32, err32=err32, bound=bound,
                hbounds=[_bound(a, b) for a, b in zip(hs64, hs32)], Hp=Hp)


def fp32_result(c, **defect):
    """(z, hidden_out buffers or None) as a kernel that computes exactly the fp32 torch-CPU formulation would leave them --
    what the checker's own test starts from; `defect`: the arguments of forward() that break it"""
    p = prepared(c)
    zl = p["z"][: c.M]
    cl = None if p["ctx"] is None else p["ctx"][: c.M]
    gl = None if p["gates"] is None else [gt[: c.M] for gt in p["gates"]]
    t32, hs32 = forward(c, zl, p["w"], cl, gl, torch.float32, **defect)
    z = p["z"].clone()
    z[: c.M, c.off_trans: c.off_trans + c.n_trans] = t32
    hidden = None
    if c.mode in ("hidden_out", "gate"):
        hidden = []
        for l, h in enumerate(hs32):
            buf = torch.full((c.M + EXTRA_ROWS, p["Hp"] + HIDDEN_SLACK), SENTINEL)
            buf[: c.M, : p["Hp"]] = 0.0
            buf[: c.M, : c.hidden[l]] = h
            hidden.append(buf)
    return z, hidden


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def measure(got_z, got_hidden, c):
    """the figures check() compares: dict(err, err32, bound, hidden=[(err, err32, bound)])"""
    p = prepared(c)
    got = got_z[: c.M, c.off_trans: c.off_trans + c.n_trans].double()
    out = dict(err=(got - p["ref64"]).abs().max().item(), err32=p["err32"], bound=p["bound"], hidden=[])
    for l, buf in enumerate(got_hidden or []):
        e = (buf[: c.M, : c.hidden[l]].double() - p["hs64"][l]).abs().max().item()
        out["hidden"].append((e,) + p["hbounds"][l])
    return out


def check(got_z, got_hidden, c):
    """the violated conditions (an empty list: the launch is right).  got_z: the row buffer [M + EXTRA_ROWS, ldz] after the
    launch, got_hidden: the hidden_out buffers [M + EXTRA_ROWS, Hp + HIDDEN_SLACK] after it (None where the mode has none);
    CPU fp32 tensors."""
    p = prepared(c)
    bad = []
    _, tmask = segment_masks(c)
    if tuple(got_z.shape) != tuple(p["z"].shape):
        return [f"z has shape {tuple(got_z.shape)}, not {tuple(p['z'].shape)}"]
    # the transformed columns against fp64
    got = got_z[: c.M, c.off_trans: c.off_trans + c.n_trans].double()
    if torch.isnan(got).any():
        bad.append(f"NaN in {int(torch.isnan(got).sum())} transformed elements")
    err = (got - p["ref64"]).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if err.max().item() > p["bound"]:
        r, k = divmod(int(err.argmax()), c.n_trans)
        bad.append(f"transformed columns: error {err.max().item():.3e} above the bound {p['bound']:.3e} (err32 {p['err32']:.3e}) "
                   f"at row {r}, transformed column {k}")
    # nothing else moves, bit for bit
    moved = (_bits(got_z) != _bits(p["z"])) & ~tmask
    if moved.any():
        r, k = divmod(int(moved.reshape(-1).to(torch.uint8).argmax()), c.ldz)
        bad.append(f"{int(moved.sum())} elements outside the transformed segment changed, the first at row {r}, column {k}")
    # hidden_out
    wants_hidden = c.mode in ("hidden_out", "gate")
    if wants_hidden != (got_hidden is not None):
        bad.append("hidden_out buffers " + ("missing" if wants_hidden else "given for a mode that has none"))
    for l, buf in enumerate(got_hidden or []):
        h, Hp = c.hidden[l], p["Hp"]
        val = buf[: c.M, :h].double()
        e = (val - p["hs64"][l]).abs()
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        err32, bound = p["hbounds"][l]
        if e.max().item() > bound:
            r, k = divmod(int(e.argmax()), h)
            bad.append(f"hidden_out[{l}]: error {e.max().item():.3e} above the bound {bound:.3e} (err32 {err32:.3e}) at row {r}, unit {k}")
        if not (buf[: c.M, h:Hp] == 0).all():
            bad.append(f"hidden_out[{l}]: the padded units' columns [{h}, {Hp}) are not zero")
        if not (_bits(buf[: c.M, Hp:]) == _bits(torch.full_like(buf[: c.M, Hp:], SENTINEL))).all():
            bad.append(f"hidden_out[{l}]: columns >= {Hp} written")
        if not (_bits(buf[c.M:]) == _bits(torch.full_like(buf[c.M:], SENTINEL))).all():
            bad.append(f"hidden_out[{l}]: rows >= M written")
    return bad


# ---- the descriptor, from the header's padding contract -----------------------------------------------------------------------------
def _padded(W, rows, cols):
    out = torch.zeros(rows, cols, dtype=torch.float32)
    out[: W.shape[0], : W.shape[1]] = W
    return out


def _padded_vec(v, n):
    out = torch.zeros(n, dtype=torch.float32)
    out[: v.numel()] = v
    return out


def split3(W):
    """three bf16 planes [3, rows, cols] with p1 + p2 + p3 == W: round-to-nearest residual split"""
    p1 = W.to(torch.bfloat16)
    r = W - p1.float()
    p2 = r.to(torch.bfloat16)
    p3 = (r - p2.float()).to(torch.bfloat16)
    return torch.stack([p1, p2, p3])


def k_permutation(Hp):
    """usf_coupling_desc: "position 8g+j holds unit 4g+j (j<4) or 16+4g+(j-4) (j>=4)" inside every block of 32"""
    unit = []
    for b in range(0, Hp, 32):
        for pos in range(32):
            g, j = divmod(pos, 8)
            unit.append(b + (4 * g + j if j < 4 else 16 + 4 * g + (j - 4)))
    return torch.tensor(unit)


@functools.lru_cache(maxsize=None)
def images(n_pass, hidden, n_trans, split):
    """the weight images of one weight set as the header asks for them (CPU tensors): fp32 W_in [Hp, ceil32(n_pass)],
    W_hid [Hp, Hp], W_out [ceil32(n_trans), Hp], vectors of Hp / ceil32(n_trans), all zero outside their true extents; split:
    the three bf16 planes of each, split_hid / split_out with the K permutation"""
    w = weights(n_pass, hidden, n_trans)
    nh = len(hidden)
    Hp, Kp, Np = padded_width(max(hidden)), ceil_to(n_pass, 32), ceil_to(n_trans, 32)
    im = dict(Hp=Hp, W_in=_padded(w["Ws"][0], Hp, Kp), b_in=_padded_vec(w["bs"][0], Hp),
              W_hid=[_padded(w["Ws"][l], Hp, Hp) for l in range(1, nh)], b_hid=[_padded_vec(w["bs"][l], Hp) for l in range(1, nh)],
              W_out=_padded(w["Ws"][nh], Np, Hp), b_out=_padded_vec(w["bs"][nh], Np),
              W_ctx=_padded_vec(w["Wc"], Hp), b_ctx=_padded_vec(w["bc"], Hp))
    if split:
        perm = k_permutation(Hp)
        im["split_in"] = split3(im["W_in"])
        im["split_hid"] = [split3(W[:, perm]) for W in im["W_hid"]]
        im["split_out"] = split3(im["W_out"][:, perm])
    return im


def case_images(c):
    return images(c.n_pass, c.hidden, c.n_trans, c.family == "bf16x3")


def descriptor(c, ptr, desc_type):
    """the usf_coupling_desc of a case; ptr(name) gives the address of the buffer `name` ("z", "W_in", "b_hid0", "split_hid1",
    "hidden_out2", "gate0", "context", ...), desc_type is the binding's CouplingDesc"""
    im = case_images(c)
    nh = len(c.hidden)
    d = desc_type()
    d.z = d.out = ptr("z")
    d.ldz = d.ldo = c.ldz
    d.M = c.M
    d.off_pass, d.n_pass, d.off_trans, d.n_trans = c.off_pass, c.n_pass, c.off_trans, c.n_trans
    d.n_hidden = nh
    for l, h in enumerate(c.hidden):
        d.hidden[l] = h
    d.W_in, d.ldw_in, d.b_in = ptr("W_in"), im["W_in"].shape[1], ptr("b_in")
    for l in range(nh - 1):
        d.W_hid[l], d.ldw_hid[l], d.b_hid[l] = ptr(f"W_hid{l}"), im["Hp"], ptr(f"b_hid{l}")
    d.W_out, d.ldw_out, d.b_out = ptr("W_out"), im["Hp"], ptr("b_out")
    d.sign, d.slope, d.act = c.sign, c.slope, c.act
    if c.mode == "ctx":
        d.context, d.W_ctx, d.b_ctx = ptr("context"), ptr("W_ctx"), ptr("b_ctx")
    if c.family == "bf16x3":
        tri = lambda P: (P.shape[2], P.shape[1] * P.shape[2])          # noqa: E731  (leading dimension, plane stride)
        d.split_in = ptr("split_in")
        d.split_in_ld, d.split_in_plane = tri(im["split_in"])
        for l in range(nh - 1):
            d.split_hid[l] = ptr(f"split_hid{l}")
            d.split_hid_ld, d.split_hid_plane = tri(im["split_hid"][l])
        d.split_out = ptr("split_out")
        d.split_out_ld, d.split_out_plane = tri(im["split_out"])
    if c.mode in ("hidden_out", "gate"):
        for l in range(nh):
            d.hidden_out[l] = ptr(f"hidden_out{l}")
        d.ld_hidden_out = im["Hp"] + HIDDEN_SLACK
    if c.mode == "gate":
        for l in range(nh):
            d.gate[l] = ptr(f"gate{l}")
        d.ld_gate = im["Hp"] + GATE_SLACK
    return d


def fake_ptr(name):
    """16-byte aligned addresses that are never read (usf_coupling_variant and the argument checks are host-only)"""
    return 0x100000 + 0x10000 * (sum(name.encode()) % 251)


@contextlib.contextmanager
def tiny_kernel_off():
    """library knob coupling_tiny = 0 for the block: the exact-f32 cases with M <= 256 and everything <= 64 would otherwise go to
    the tiny-layer kernel (tests/test_gm_live.py does the same)"""
    from usflows_amd.config import config
    old = config.get_lib("coupling_tiny", 1)
    config.set_lib("coupling_tiny", 0)
    try:
        yield
    finally:
        config.set_lib("coupling_tiny", old)


def variant(c, lib, desc_type):
    """usf_coupling_variant of the case's descriptor (host-only)"""
    return lib.usf_coupling_variant(ctypes.byref(descriptor(c, fake_ptr, desc_type)))

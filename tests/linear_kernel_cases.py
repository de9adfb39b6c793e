"""The three kernel families behind usf_linear_f32 -- the small-batch kernel (usf_linear_skinny.hip: linear_skinny_kernel<SK_G>
with mw waves along M and ks K ranges), the exact-f32 tile (usf_linear.hip: linear_kernel<TM,TN,WM,BK,PRO,EPI>, tiles 2122 / 2244 /
2254) and the bf16x3 tile (usf_linear_bf16x3.hip: linear_bf16x3_kernel<TN,WM,PRO,NB,SIDE>, tiles 3244 / 3442 / 3542 / 3584) -- one
launch at a time against fp64: the case table, a descriptor builder that knows nothing but the header's contract
(include/usflows_hip.h, usf_linear_desc, and the A_planes_out paragraph of include/usflows_hip_internal.h; the W_split planes are
split by hand, no engine packer is involved), the layer in fp64 / fp32 on the CPU in the header's order and the checker.
Importable without a GPU: tests/test_linear_kernels_cpu.py holds the table and the checker to account,
tests/test_linear_kernels_gpu.py launches.

Buffers.  Every buffer has slack: EXTRA_ROWS rows below M, lda > K, ldw > K, ldc > N, ldr / ldadd > N, vectors longer than their
extent.  A NaN with a payload of its own sits in every element the contract does not let a launch read into a result (A and W
columns >= K, rows >= M resp. >= N, residual / addend / gate columns >= N, bias / post_mul past N, pre_div / pre_sub past K,
W_split columns past ceil32(K)) and in every element of C (the launch must overwrite C[:M, :N] and nothing else).  Zero stands
only where the header demands it: W_split columns [K, ceil32(K)), and the A_planes_out image the caller hands over.

What the table holds (tests/test_linear_kernels_cpu.py enforces each line):
 * small-batch kernel, default knobs, M <= 768: SK_G = 4 at all eight (mw, ks) in {1, 2} x {1, 2, 3, 4}; every M of SK_M (the
   16-row tile switch, the mw switch at 32 / 33, the second block row at 65, the limit 768), every N of SK_N (the 16-feature
   block edge, partial 16-byte stores), every K of SK_K (ks 1..4, a ragged last step, unequal steps per K-range wave; K = 528 and
   784: 3 and 4 fetch groups, one more in wave 0 than in the others); the five epilogue forms of FIVE_FORMS at both mw; both
   vec_ok; every prologue; two SK_G = 8 cases (knob skinny_g = 8, one per mw); two skinny_ks_small = 8 cases at mw = 1, one with
   ks = 8 and one where nstep caps it (K = 80: ks = 5).
 * exact-f32 tiles, knob skinny_max = 0: all of tile x PRO x EPI x vec_ok (36 instantiation keys: 18 kernels, each on both store
   paths); EPI 2 as addend and as gate on every tile; the prologue as div only, sub only and both; bias_vec both ways (N % 4 == 0
   with an aligned bias, and not); every K of F32_K (one, two and three-plus 16-k slabs, the last slab holding one or two 8-k
   steps); tile 2122 at every M of F32_M_SMALL and N of F32_N_SMALL, the 256-row tiles at every M of F32_M_BIG, tile 2244 at every
   N of F32_N_2244, tile 2254 at every N of F32_N_2254; one case per 256-row tile with nine row panels (M = 2100: the block map
   panel = (seq / nbn) * 8 + xcd takes its second round and its early return).
 * bf16x3 tiles, knob skinny_max = 0: per tile the five forms of FIVE_FORMS on the plain template, two on PRO (div + sub, sub
   only) and two on SIDE (bias, addend + leaky); K cycles through B3_K (1..5 slabs of 32, ragged and full, against rings of 2 and
   4 weight buffers); N % 4 == 0 with a ragged last column block; tile 3244 at M in {65, 129, 257, 769, 1025}; the other three at
   the smallest shapes the dispatcher gives them (B3_SHAPES; profiles/linear_kernel_parity.md says why they cannot be smaller)."""
import collections
import contextlib
import ctypes
import functools

import torch

from coupling_kernel_cases import ceil_to, split3, _bits      # noqa: F401  (re-exported for the tests)

ACT_NONE, ACT_LEAKY_RELU, ACT_GATE = 0, 1, 2          # include/usflows_hip.h: USF_ACT_*
EXTRA_ROWS = 3                                        # rows below M (below N in W) in every row buffer
SENTINEL = 9.0                                        # the row between the planes of an A_planes_out buffer

Case = collections.namedtuple("Case", "family M N K form pro bias_al vec side knobs")

# the epilogue forms: bias, activation, slope, the [M, N] operand (residual / addend / gate), res_sign, post_mul
Form = collections.namedtuple("Form", "bias act slope extra res_sign post_mul")
FORMS = {
    "plain": Form(False, ACT_NONE, 0.0, None, 1.0, False),
    "bias": Form(True, ACT_NONE, 0.0, None, 1.0, False),
    "bias_leaky": Form(True, ACT_LEAKY_RELU, 0.01, None, 1.0, False),
    "bias_relu": Form(True, ACT_LEAKY_RELU, 0.0, None, 1.0, False),
    "residual": Form(True, ACT_LEAKY_RELU, 0.2, "residual", -1.0, True),      # every later step of the header's order at work
    "residual_plus": Form(False, ACT_NONE, 0.0, "residual", 1.0, False),
    "addend_leaky": Form(True, ACT_LEAKY_RELU, 0.01, "addend", 1.0, False),
    "gate": Form(True, ACT_GATE, 0.01, "gate", 1.0, False),
    "post_mul": Form(True, ACT_NONE, 0.0, None, 1.0, True),
}
FIVE_FORMS = ["bias_leaky", "residual", "addend_leaky", "gate", "post_mul"]
PROS = ["none", "div", "sub", "both"]

SK_M = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 100, 768]
SK_N = [1, 3, 4, 15, 16, 17, 20, 33, 161]
SK_K = [4, 16, 20, 32, 36, 48, 52, 64, 260, 528, 784]
SK_CYCLED = 65

F32_K = [4, 8, 12, 16, 20, 36, 52, 100]
F32_M_SMALL, F32_N_SMALL = [1, 31, 33, 64, 130, 800], [1, 3, 4, 33, 63, 64]
F32_M_BIG = [65, 255, 256, 257, 520]
F32_N_2244 = [68, 100, 128, 161, 250, 256]       # (161 pads less on 128-wide blocks: 95 against 159 columns)
F32_N_2254 = [129, 160, 300]
F32_TILES = {2122: (F32_M_SMALL, F32_N_SMALL), 2244: (F32_M_BIG, F32_N_2244), 2254: (F32_M_BIG, F32_N_2254)}
NINE_PANELS = 2100

B3_K = [8, 40, 64, 72, 104, 136]
B3_M_3244, B3_N_3244 = [65, 129, 257, 769, 1025], [68, 100, 128, 196]
# the smallest [M, N] the dispatcher hands to each of the other tiles: 256 tiles of 128 x 160 before it leaves 3244
B3_SHAPES = {3442: [(32641, 68), (32641, 124)], 3584: [(32641, 156), (32641, 132)], 3542: [(1921, 2692)]}
# (template, form, prologue) of the nine cases of a bf16x3 tile
B3_NINE = [("plain", f, "none") for f in FIVE_FORMS] + [("PRO", "bias_leaky", "both"), ("PRO", "post_mul", "sub"),
                                                        ("SIDE", "bias", "none"), ("SIDE", "addend_leaky", "none")]
TILES_OFF = (("skinny_max", 0),)                  # the tiled kernels at any M


def _build_cases():
    cases = []
    # small-batch kernel: M, N, K, form cycle with pairwise coprime periods (13, 9, 11, 5); vec_ok, prologue and the bias
    # alignment with periods 2, 4, 3
    for i in range(SK_CYCLED):
        cases.append(Case("skinny", SK_M[i % 13], SK_N[i % 9], SK_K[i % 11], FIVE_FORMS[i % 5], PROS[(i // 2) % 4], i % 3 != 0,
                          i % 2 == 0, False, ()))
    cases += [Case("skinny", 31, 20, 784, "addend_leaky", "none", True, True, False, (("skinny_g", 8),)),
              Case("skinny", 65, 33, 528, "residual", "both", False, False, False, (("skinny_g", 8),)),
              Case("skinny", 17, 20, 260, "gate", "none", True, True, False, (("skinny_ks_small", 8),)),
              Case("skinny", 32, 17, 80, "residual", "sub", False, False, False, (("skinny_ks_small", 8),))]
    # exact-f32 tiles: tile x PRO x EPI x vec_ok, shapes cycling through the tile's lists
    for code, (ms, ns) in F32_TILES.items():
        j = 0
        for pro in (0, 1):
            for epi in (0, 1, 2):
                for vec in (0, 1):
                    M, N, K = ms[j % len(ms)], ns[(j + j // len(ms)) % len(ns)], F32_K[(j + code // 10) % 8]
                    form = (["bias_leaky", "post_mul", "plain", "bias_relu"][j % 4] if epi == 0 else
                            ("residual", "residual_plus")[vec] if epi == 1 else ("addend_leaky", "gate")[vec ^ pro])
                    cases.append(Case("f32", M, N, K, form, PROS[1 + j % 3] if pro else "none", j % 2 == 0, bool(vec), False, TILES_OFF))
                    j += 1
    cases += [Case("f32", NINE_PANELS, 256, 36, "bias_leaky", "none", True, True, False, TILES_OFF),
              Case("f32", NINE_PANELS, 129, 52, "residual", "both", False, False, False, TILES_OFF)]
    # bf16x3 tiles: nine cases each, K with period 6 against them
    i = 0
    for code in (3244, 3442, 3542, 3584):
        for template, form, pro in B3_NINE:
            M, N = (B3_M_3244[i % 5], B3_N_3244[i % 4]) if code == 3244 else B3_SHAPES[code][i % len(B3_SHAPES[code])]
            cases.append(Case("bf16x3", M, N, B3_K[i % 6], form, pro, i % 2 == 0, True, template == "SIDE", TILES_OFF))
            i += 1
    return cases


CASES = _build_cases()


def case_id(c):
    return (f"{c.family}-M{c.M}-N{c.N}-K{c.K}-{c.form}-pro_{c.pro}-{'b16' if c.bias_al else 'b4'}-{'vec' if c.vec else 'novec'}"
            + ("-side" if c.side else "") + "".join(f"-{k}{v}" for k, v in c.knobs))


# ---- which kernel a case runs: the dispatchers' rules restated (usf_linear_variant is the arbiter, in the CPU test) ----------------
def f32_tile(M, N):
    if M <= 64 or N <= 64:
        return 2122
    return 2254 if ceil_to(N, 160) - N < ceil_to(N, 128) - N else 2244


def bf16x3_tile(M, N):
    if ceil_to(M, 128) // 128 * (ceil_to(N, 160) // 160) < 256:
        return 3244
    if ceil_to(N, 160) - N < ceil_to(N, 128) - N:
        big = M >= 2048
        if big:
            rounds = ceil_to(M, 256) // 256 * (ceil_to(N, 160) // 160) / 256.0
            frac = rounds - int(rounds)
            if rounds > 1.0 and 0.0 < frac < 0.7:
                big = False
        return 3584 if big else 3542
    return 3442


def skinny_shape(c):
    """(SK_G, mw, ks) by the rule of linear_skinny_dispatch: two wave rows above 32 rows, ks = 4 (mw = 1: skinny_ks_small, 1..8)
    K ranges capped by the number of 16-k steps"""
    knobs = dict(c.knobs)
    mw = 2 if c.M > 32 else 1
    small = knobs.get("skinny_ks_small", 4)
    if not 1 <= small <= 8:
        small = 4
    ks = min(small if mw == 1 else 4, ceil_to(c.K, 16) // 16)
    return (8 if knobs.get("skinny_g", 4) == 8 else 4), mw, ks


def layout(c):
    """leading dimensions and vector offsets of a case's buffers"""
    kp = ceil_to(c.K, 32)
    ldc = ceil_to(c.N, 4) + 4 if c.vec else c.N + (1 if (c.N + 1) % 4 else 2)
    ldx = ceil_to(c.N, 4) + 4 if c.family == "bf16x3" else c.N + 5
    return dict(lda=c.K + 4, ldw=c.K + 8, ldc=ldc, ldx=ldx, ldws=kp + 8, ldp=kp + 8, b_off=0 if c.bias_al else 1)


def store_vec_ok(c):
    return int(layout(c)["ldc"] % 4 == 0)          # (C itself is 16-byte aligned in every case)


def instantiation(c):
    """the key of the kernel instantiation a case runs: (family, variant code of usf_linear_variant, ...) with
    (SK_G, mw, ks) for the small-batch kernel, (PRO, EPI, vec_ok) for the exact-f32 tile, (template, epilogue) for bf16x3"""
    f = FORMS[c.form]
    if c.family == "skinny":
        return ("skinny", 1000) + skinny_shape(c)
    if c.family == "f32":
        epi = 1 if f.extra == "residual" else (2 if f.extra in ("addend", "gate") else 0)
        return "f32", f32_tile(c.M, c.N), int(c.pro != "none"), epi, store_vec_ok(c)
    return "bf16x3", bf16x3_tile(c.M, c.N), ("SIDE" if c.side else "PRO" if c.pro != "none" else "plain"), c.form


# ---- buffers, the layer in fp64 / fp32 ----------------------------------------------------------------------------------------------
def _seed(*ints):
    s = 54321
    for v in ints:
        s = (s * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return s


def nan_like(rows, cols, salt):
    """quiet NaNs with a payload of their own each (and a range of payloads per buffer: `salt`): a NaN that moved is another NaN"""
    lin = torch.arange(rows * cols, dtype=torch.int64).reshape(rows, cols)
    return (0x7FC00000 + 1 + (lin + salt * 0x50001) % 0x3FFFFE).to(torch.int32).view(torch.float32)


def nan_like_bf16(shape):
    n = 1
    for s in shape:
        n *= s
    return (0x7FC0 + 1 + torch.arange(n, dtype=torch.int64) % 0x3E).to(torch.int16).view(torch.bfloat16).reshape(shape)


def _poisoned(values, rows, cols, salt):
    out = nan_like(rows, cols, salt)
    out[: values.shape[0], : values.shape[1]] = values
    return out


def forward(c, p, dtype, defect=None):
    """the layer in `dtype`, in the header's order: prologue A / pre_div - pre_sub, GEMM, + bias, + addend, activation (or the
    gate v * (h > 0 ? 1 : slope)), residual + res_sign * v, * post_mul.  `defect`: one of DEFECTS (for the checker's own test)"""
    f, L = FORMS[c.form], layout(c)
    M, N, K = c.M, c.N, c.K
    a = p["A"][:M, :K].to(dtype)
    if c.pro in ("div", "both"):
        a = a / p["pre_div"][:K].to(dtype)
    if c.pro in ("sub", "both"):
        a = a - p["pre_sub"][:K].to(dtype)
    W = p["W"][:N, :K].to(dtype)
    if defect == "drop_last_kstep":
        keep = (K - 1) // 8 * 8
        a, W = a[:, :keep], W[:, :keep]
    v = a @ W.t()
    if f.bias:
        v = v + p["bias"][L["b_off"]: L["b_off"] + N].to(dtype)
    ex = None if f.extra is None else p["extra"][:M, :N].to(dtype)
    pm = p["post_mul"][:N].to(dtype) if f.post_mul else None

    def act(x):
        return torch.where(x > 0, x, x * f.slope) if f.act == ACT_LEAKY_RELU else x

    if f.extra == "addend" and defect != "addend_after_act":
        v = v + ex
    if f.act == ACT_GATE:
        v = v * torch.where((ex >= 0) if defect == "gate_positive_at_zero" else (ex > 0), 1.0, f.slope).to(dtype)
    elif defect != "act_after_residual":
        v = act(v)
    if f.extra == "addend" and defect == "addend_after_act":
        v = v + ex
    if f.extra == "residual":
        if defect == "post_mul_before_residual" and pm is not None:
            v, pm = v * pm, None
        v = ex + (1.0 if defect == "ignore_res_sign" else f.res_sign) * v
        if defect == "act_after_residual":
            v = act(v)
    if pm is not None:
        v = v * pm
    return v


DEFECTS = ["drop_last_kstep", "act_after_residual", "post_mul_before_residual", "addend_after_act", "gate_positive_at_zero",
           "ignore_res_sign"]


def _bound(ref64, ref32):
    """(err32, bound): max(4 err32, 2e-6 max(1, max |ref|)) -- the rule of test_linear_parity and of the coupling-kernel tests;
    err32 = the error of the fp32 torch-CPU evaluation of the same values"""
    err32 = (ref32.double() - ref64).abs().max().item()
    return err32, max(4 * err32, 2e-6 * max(1.0, ref64.abs().max().item()))


@functools.lru_cache(maxsize=4)
def prepared(c):
    """buffers and references of a case (CPU tensors): A [M + 3, lda], W [N + 3, ldw], bias [N + 8] (the vector starts at b_off),
    pre_div / pre_sub [K + 4], extra (residual / addend / gate) [M + 3, ldx], post_mul [N + 4], C0 [M + 3, ldc] (what C holds
    before the launch: NaN everywhere), W_split [3, N + 1, ldws] bf16, planes0 [3, ceil32(M) + 1, ldp] bf16 (zeros, a sentinel row
    behind every plane); ref64 / ref32 [M, N], err32, bound"""
    f, L = FORMS[c.form], layout(c)
    M, N, K = c.M, c.N, c.K
    g = torch.Generator().manual_seed(_seed(M, N, K, len(c.form), len(c.pro), c.bias_al, c.vec, c.side))
    rows = M + EXTRA_ROWS
    p = dict(A=_poisoned(torch.randn(M, K, generator=g), rows, L["lda"], 1),
             W=_poisoned(torch.randn(N, K, generator=g) / K ** 0.5, N + EXTRA_ROWS, L["ldw"], 2),
             C0=nan_like(rows, L["ldc"], 3))
    if f.bias:
        p["bias"] = nan_like(1, N + 8, 4)[0].contiguous()
        p["bias"][L["b_off"]: L["b_off"] + N] = torch.randn(N, generator=g)
    if c.pro in ("div", "both"):
        # |pre_div| in [0.5, 1.5) with either sign (ScaleTransform's scale)
        dv = (torch.rand(K, generator=g) + 0.5) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
        p["pre_div"] = _poisoned(dv[None], 1, K + 4, 5)[0].contiguous()
    if c.pro in ("sub", "both"):
        p["pre_sub"] = _poisoned(torch.randn(1, K, generator=g), 1, K + 4, 6)[0].contiguous()
    if f.extra is not None:
        ex = torch.randn(M, N, generator=g)
        if f.extra == "gate":
            # a saved layer output: exact zeros of either sign among the values (a gate of 0 takes the slope)
            u = torch.rand(M, N, generator=g)
            ex = torch.where(u < 0.1, torch.zeros(()), ex)
            ex = torch.where(u < 0.05, -torch.zeros(()), ex)
            ex[-1, -1] = 0.0
        p["extra"] = _poisoned(ex, rows, L["ldx"], 7)
    if f.post_mul:
        pm = (torch.rand(N, generator=g) + 0.5) * torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
        p["post_mul"] = _poisoned(pm[None], 1, N + 4, 8)[0].contiguous()
    if c.family == "bf16x3":
        # three planes of W as the header words them: round-to-nearest residual split, zero in [K, ceil32(K)); NaN beyond, and
        # in the row between two planes
        kp = ceil_to(K, 32)
        ws = nan_like_bf16((3, N + 1, L["ldws"]))
        ws[:, :N, :kp] = 0
        ws[:, :N, :K] = split3(p["W"][:N, :K].contiguous())
        p["W_split"] = ws
    if c.side:
        mp = ceil_to(M, 32)
        p["planes0"] = torch.zeros(3, mp + 1, L["ldp"], dtype=torch.bfloat16)
        p["planes0"][:, mp] = SENTINEL
    p["ref64"] = forward(c, p, torch.float64)
    p["ref32"] = forward(c, p, torch.float32)
    p["err32"], p["bound"] = _bound(p["ref64"], p["ref32"])
    return p


INPUTS = ["A", "W", "bias", "pre_div", "pre_sub", "extra", "post_mul", "W_split"]          # buffers a launch only reads


def with_result(c, values):
    """C as a launch that computes `values` [M, N] would leave it"""
    C = prepared(c)["C0"].clone()
    C[: c.M, : c.N] = values.to(torch.float32)
    return C


def fp32_result(c):
    """C as a kernel that computes exactly the fp32 torch-CPU formulation would leave it"""
    return with_result(c, prepared(c)["ref32"])


# ---- the checker ------------------------------------------------------------------------------------------------------------------
def measure(got_C, c):
    """the figures check() compares: dict(err, err32, bound)"""
    p = prepared(c)
    err = (got_C[: c.M, : c.N].double() - p["ref64"]).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return dict(err=err.max().item(), err32=p["err32"], bound=p["bound"])


def check(got_C, c):
    """the violated conditions (an empty list: the launch is right).  got_C: the buffer [M + EXTRA_ROWS, ldc] after the launch, a
    CPU fp32 tensor: C[:M, :N] within the bound of fp64, every other element as it was, bit for bit"""
    p = prepared(c)
    bad = []
    if tuple(got_C.shape) != tuple(p["C0"].shape):
        return [f"C has shape {tuple(got_C.shape)}, not {tuple(p['C0'].shape)}"]
    got = got_C[: c.M, : c.N].double()
    if torch.isnan(got).any():
        bad.append(f"NaN in {int(torch.isnan(got).sum())} elements of C[:M, :N]")
    err = (got - p["ref64"]).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if err.max().item() > p["bound"]:
        r, k = divmod(int(err.argmax()), c.N)
        bad.append(f"C: error {err.max().item():.3e} above the bound {p['bound']:.3e} (err32 {p['err32']:.3e}) at row {r}, column {k}")
    moved = _bits(got_C) != _bits(p["C0"])
    moved[: c.M, : c.N] = False
    if moved.any():
        r, k = divmod(int(moved.reshape(-1).to(torch.uint8).argmax()), got_C.shape[1])
        bad.append(f"{int(moved.sum())} elements outside C[:M, :N] changed, the first at row {r}, column {k}")
    return bad


# ---- the descriptor, from the header's contract ---------------------------------------------------------------------------------------
def descriptor(c, ptr, desc_type, side=None):
    """the usf_linear_desc of a case; ptr(name) gives the address of the buffer `name` ("A", "W", "bias", "pre_div", "pre_sub",
    "extra", "post_mul", "C", "W_split", "planes"), desc_type is the binding's LinearDesc; side: overrides the case's A_planes_out"""
    f, L = FORMS[c.form], layout(c)
    d = desc_type()
    d.A, d.lda, d.W, d.ldw, d.C, d.ldc = ptr("A"), L["lda"], ptr("W"), L["ldw"], ptr("C"), L["ldc"]
    d.M, d.N, d.K = c.M, c.N, c.K
    if f.bias:
        d.bias = ptr("bias") + 4 * L["b_off"]
    if c.pro in ("div", "both"):
        d.pre_div = ptr("pre_div")
    if c.pro in ("sub", "both"):
        d.pre_sub = ptr("pre_sub")
    if f.extra == "residual":
        d.residual, d.ldr = ptr("extra"), L["ldx"]
    elif f.extra is not None:
        d.addend, d.ldadd = ptr("extra"), L["ldx"]
    if f.post_mul:
        d.post_mul = ptr("post_mul")
    d.res_sign, d.slope, d.act = f.res_sign, f.slope, f.act
    if c.family == "bf16x3":
        d.W_split, d.ldw_split, d.split_plane_stride = ptr("W_split"), L["ldws"], (c.N + 1) * L["ldws"]
    if c.side if side is None else side:
        d.A_planes_out, d.ldp_out, d.planes_out_stride = ptr("planes"), L["ldp"], (ceil_to(c.M, 32) + 1) * L["ldp"]
    return d


def fake_ptr(name):
    """16-byte aligned addresses that are never read (usf_linear_variant is host-only)"""
    return 0x100000 + 0x100000 * (sum(name.encode()) % 251)


@contextlib.contextmanager
def knobs(pairs):
    """the library's tuning knobs `pairs` ((name, value), ...) set for the block and put back afterwards (as
    coupling_kernel_cases.tiny_kernel_off does for coupling_tiny)"""
    from usflows_amd.config import config
    defaults = {"skinny_max": 768, "skinny_g": 4, "skinny_ks_small": 4}
    old = [(name, config.get_lib(name, defaults[name])) for name, _ in pairs]
    for name, value in pairs:
        config.set_lib(name, value)
    try:
        yield
    finally:
        for name, value in old:
            config.set_lib(name, value)


def variant(c, lib, desc_type):
    """usf_linear_variant of the case's descriptor under the case's knobs (host-only)"""
    with knobs(c.knobs):
        return lib.usf_linear_variant(ctypes.byref(descriptor(c, fake_ptr, desc_type)))

"""The weight-gradient kernels of F.linear -- wgrad_kernel, wgrad_bf16x3_kernel, wgrad_lw_kernel with wl_mfma_loop<NI, NJ, CS>,
grad_jobs_kernel, reduce_partials_kernel, colsum_kernel (usf_train.hip) and wgrad_planes_kernel<BLK> with
wp_mfma_loop<NI, NJ, CS, BLK>, reduce_partials_cls_kernel, reduce_partials_cls_jobs_kernel, split_planes_kernel
(usf_wgrad_planes.hip) -- one launch at a time against fp64: the case tables, the launch rules restated from the sources
(usf_wgrad_variant, pick_splits, the rows per range, ni / nj -> instantiation, the planes schedule's classes, fold flags and
partial counts), buffer builders that know nothing but include/usflows_hip_internal.h, the sums in fp64 / fp32 on the CPU and the
checkers.  Importable without a GPU: tests/test_wgrad_kernels_cpu.py holds the tables, the restated rules and the checkers to
account, tests/test_wgrad_kernels_gpu.py launches.

Buffers.  Every buffer has slack and a guard in front of and behind it.  A NaN with a payload of its own sits wherever the
contract keeps a launch from reading into a result or from writing: columns [N, ld) of Y and [K, ld) of A (fp32 and planes
alike), rows >= M of the fp32 operands, columns of the planes outside [off, off + N), blocks outside [kb0, kb0 + ceil(N / 32))
and the positions >= N of the last block, G outside [N, K], colsum_out beyond N, the whole workspace, G itself where beta == 0.
Zeros stand only where a header demands them: rows [M, ceil32(M)) of row-major planes, the padding rows of a blocked Y (those
of a blocked A hold finite junk).  The workspace handed over is EXACTLY what the matching *_workspace_floats call reports, a
NaN guard behind it.

Bound (the project's GEMM rule with the reduction length M in place of 32 nk, applied to EVERY element of G[:N, :K] and every
column sum): err <= max(4 err32, 6e-8 sqrt(M)) relative to max |ref64|, err32 the same sum in fp32 on the CPU accumulated slab
by slab and range by range as the case's plan says.  Census cases are compared bit for bit."""
import collections
import contextlib
import functools
import math

import torch

from planes_kernel_cases import bits16, bits32, ceil_to, from_chunks, nan_bits16, nan_f32, split_planes, to_chunks  # noqa: F401

GF = 512                       # floats of NaN in front of and behind every fp32 buffer (2 KiB: bases stay 16-byte aligned)
GH = 1024                      # the same for bf16 buffers, in elements
EXTRA_ROWS = 3                 # NaN rows below M in row-major fp32 operands
CUS = 256                      # the table is written for this many compute units
KEPT = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]          # (Y plane, A plane), in the kernels' order
TUNING_DEFAULTS = {"wgrad_lw_min": 8192, "wgrad_blocks": 768, "wgrad_sched": 1, "wgrad_fold": 1, "wgrad_rounds": 3, "wgrad_old": 0}


@contextlib.contextmanager
def knobs(pairs):
    """the library's weight-gradient tuning knobs `pairs` set for the block and put back afterwards (planes_kernel_cases.knobs
    knows the planes pipeline's knobs only)"""
    from usflows_amd.config import config
    old = [(name, config.get_lib(name, TUNING_DEFAULTS[name])) for name, _ in pairs]
    for name, value in pairs:
        config.set_lib(name, value)
    try:
        yield
    finally:
        for name, value in old:
            config.set_lib(name, value)


def cdiv(a, b):
    return -(-a // b)


def _seed(*ints):
    s = 97531
    for v in ints:
        s = (s * 1000003 + int(v) + 11) % (2 ** 31 - 1)
    return s


# =====================================================================================================================================
# the launch rules, restated from usf_train.hip and usf_wgrad_planes.hip
# =====================================================================================================================================
def wg_tiles(N, K):
    return cdiv(N, 128) * cdiv(K, 128)


def pick_splits(M, tiles, lw, blocks=768):
    """row ranges: 640 (256-thread kernels) resp. wgrad_blocks (loader waves) blocks over the tiles, ranges of >= 256 resp. 1024 rows"""
    target = (blocks if blocks >= 1 else 768) if lw else 640
    s = cdiv(target, tiles)
    s = min(s, cdiv(M, 1024) if lw else cdiv(M, 256))
    return min(max(s, 1), 256)


def wgrad_variant(M, N, K, ldy, lda, mode, lw_min=8192):
    """usf_wgrad_variant: 0 exact-f32, 1 bf16x3 (256 threads), 2 bf16x3 with loader waves"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    if mode == 1 and M >= lw_min and M * wg_tiles(N, K) >= 160000 and (M + 448) * max(ldy, lda) * 4 < 2 ** 32:
        return 2
    return 1 if mode == 1 and M >= 2048 else 0


def f32_plan(M, N, K, ldy, lda, mode, cs, kn=()):
    """what usf_wgrad_plan answers: variant, row ranges, rows per range, direct store, grid, threads, reduction launch, workspace"""
    kn = dict(kn)
    variant = wgrad_variant(M, N, K, ldy, lda, mode, kn.get("wgrad_lw_min", 8192))
    tiles = wg_tiles(N, K)
    splits = pick_splits(M, tiles, variant == 2, kn.get("wgrad_blocks", 768))
    rows = ceil_to(cdiv(M, splits), 32) or 32
    return dict(variant=variant, splits=splits, rows=rows, direct=int(splits == 1 and not cs), grid=tiles * ceil_to(splits, 8),
                threads=768 if variant == 2 else 256, reduce=int(splits > 1 or cs), need=splits * N * (K + (1 if cs else 0)))


def f32_workspace_floats(M, N, K):
    """usf_wgrad_workspace_floats: either kernel's row ranges, + the partial column sums"""
    t = wg_tiles(N, K)
    return max(pick_splits(M, t, False), pick_splits(M, t, True)) * N * (K + 1)


def plan_ranges(M, rows, splits):
    """[(m_begin, m_end)] per row range; an EMPTY range has m_begin >= m_end"""
    return [(s * rows, min(s * rows + rows, M)) for s in range(splits)]


def find_empty_range(N, K, mode, lo, hi, ld=None):
    """the smallest M in [lo, hi] at which the last row range of a usf_wgrad_f32 call comes out EMPTY, or None"""
    ld = ld or ceil_to(max(N, K), 4)
    for M in range(lo, hi + 1):
        p = f32_plan(M, N, K, ld, ld, mode, False)
        if (p["splits"] - 1) * p["rows"] >= M:
            return M
    return None


def sub_tiles(rem):
    """live 16-wide sub-tiles of a wave's 64-column patch with `rem` columns left (usf_train.hip: ni / nj)"""
    return 0 if rem <= 0 else (4 if rem >= 64 else cdiv(rem, 16))


def _pow2(n):
    return 4 if n > 2 else (2 if n > 1 else 1)


def f32_instantiations(c):
    """the code paths a usf_wgrad_f32 / _bias_f32 / grad_jobs weight case runs, as labels"""
    p = case_plan(c)
    out = set()
    for n0 in range(0, c.N, 128):
        for k0 in range(0, c.K, 128):
            for wn in (0, 1):
                for wk in (0, 1):
                    ni, nj = sub_tiles(c.N - n0 - 64 * wn), sub_tiles(c.K - k0 - 64 * wk)
                    if ni == 0 or nj == 0:
                        out.add("idle-wave")
                        continue
                    if p["variant"] == 2:
                        cs = c.cs and k0 == 0 and wk == 0 and nj == 4
                        out.add(f"lw<{_pow2(ni)},{4 if cs else _pow2(nj)}{',cs' if cs else ''}>")
                    elif p["variant"] == 1:
                        out.add(f"bf<{ni},{nj}>")
                        if c.cs and k0 == 0 and wk == 0:
                            out.add(f"bf-cs<{ni}>")
                    else:
                        out.add("f32-full" if ni == 4 and nj == 4 else f"f32-edge<{ni},{nj}>")
    if p["variant"] == 1:
        out |= {"bf-load-" + ("scalar" if n % 4 else "vector") for n in (c.N, c.K)}
        if c.N > 4:
            out.add("bf-load-vector")
    out.add("direct" if p["direct"] else "partials")
    if p["variant"] == 2 and (c.N % 2 or c.K % 2):
        out.add("lw-straddle-" + ("N" if c.N % 2 else "") + ("K" if c.K % 2 else ""))
    rg = plan_ranges(c.M, p["rows"], p["splits"])
    if any(b >= e for b, e in rg) and c.M > 0:
        out.add("empty-range")
    return out


# ---- the planes schedule (wp_schedule) ------------------------------------------------------------------------------------------------
def wp_plain_splits(M, N, K, blocks=768):
    return pick_splits(M, wg_tiles(N, K), True, blocks)


def wp_schedule(M, N, K, balanced, plain_splits, cus=CUS, fold=1, rounds=3):
    """wp_schedule restated: None where it answers false, else dict(fold flags, T / nseg / rows per class, items, blocks)"""
    cus = max(cus & ~7, 8)
    S = cdiv(M, 32)
    fN, rN = divmod(N, 128)
    fK, rK = divmod(K, 128)
    fold = balanced and fold != 0
    foldN = int(fold and fN >= 1 and 0 < rN <= 16)
    foldK = int(fold and fK >= 1 and 0 < rK <= 16)
    cn = [fN - 1 if foldN else fN, foldN, 1 if (not foldN and rN) else 0]
    T = [0] * 9
    for tn in range(3):
        for tk in range(3):
            if tn == 1:
                ck = fK if tk == 0 else ((1 if rK else 0) if tk == 2 else 0)
            else:
                ck = (fK - 1 if foldK else fK) if tk == 0 else (foldK if tk == 1 else (1 if (not foldK and rK) else 0))
            T[3 * tn + tk] = cn[tn] * ck
    tiles = sum(T)
    if tiles == 0 or S < 1:
        return None
    if balanced:
        if tiles > cus or S < 4:
            return None
        ns_max = max(rounds, 1) * cus // tiles
        ns, best = max(cus // tiles, 1), -1
        for c in range(1, min(ns_max, S, 256) + 1):
            slabs = cdiv(S, c)
            cost = cdiv(tiles * cdiv(S, slabs), cus) * (slabs + 6)
            if best < 0 or cost < best:
                best, ns = cost, c
    else:
        ns = max(plain_splits, 1)
    ns = min(ns, S, 256)
    slabs = cdiv(S, ns)
    nseg = [cdiv(S, slabs) if T[c] else 0 for c in range(9)]
    rows = [slabs * 32 if T[c] else 0 for c in range(9)]
    load = [0] * 8
    for c in range(9):
        n = T[c] * nseg[c]
        cnx = [n // 8] * 8
        for _ in range(n % 8):
            bx = 0
            for x in range(1, 8):
                if load[x] + cnx[x] < load[bx] + cnx[bx]:
                    bx = x
            cnx[bx] += 1
        load = [a + b for a, b in zip(load, cnx)]
    return dict(balanced=int(balanced), foldN=foldN, foldK=foldK, fN=fN, fK=fK, rN=rN, rK=rK, T=T, nseg=nseg, rows=rows,
                items=sum(t * s for t, s in zip(T, nseg)), blocks=8 * max(load), parts=max(nseg + [1]))


def planes_workspace_floats(M, N, K, cus=CUS, kn=()):
    kn = dict(kn)
    m = wp_plain_splits(M, N, K, kn.get("wgrad_blocks", 768))
    sc = wp_schedule(M, N, K, True, 0, cus, kn.get("wgrad_fold", 1), kn.get("wgrad_rounds", 3))
    return max(m, sc["parts"] if sc else 0) * N * (K + 1)


def planes_plan(M, N, K, workspace_floats, cus=CUS, kn=()):
    """the schedule usf_wgrad_planes_f32 / usf_wgrad_blocked_f32 launch from (what usf_wgrad_planes_plan answers)"""
    kn = dict(kn)
    sc = None
    if kn.get("wgrad_sched", 1) != 0:
        sc = wp_schedule(M, N, K, True, 0, cus, kn.get("wgrad_fold", 1), kn.get("wgrad_rounds", 3))
        if sc and sc["parts"] * N * (K + 1) > workspace_floats:
            sc = None
    return sc or wp_schedule(M, N, K, False, wp_plain_splits(M, N, K, kn.get("wgrad_blocks", 768)), cus)


CLASS_NAMES = ["nn", "nw", "ne", "wn", "ww", "we", "en", "ew", "ee"]          # (type in n)(type in k): normal / wide / edge


def planes_tile_widths(sc, cls):
    tn, tk = divmod(cls, 3)
    return ([128, 128 + sc["rN"], sc["rN"]][tn], [128, 128 + sc["rK"], sc["rK"]][tk])


def _wp_sub(width, wv, blk):
    rem = width - 64 * wv
    n = 0 if rem <= 0 else ((4 if rem >= 64 else cdiv(rem, 16)) if wv == 0 else cdiv(rem, 16))
    if blk and 0 < n < 4:
        n = (n + 1) & ~1
    return n


def _wp_round(n):
    return 5 if n > 4 else (4 if n > 2 else (2 if n > 1 else 1))


def planes_instantiations(c):
    """wp_mfma_loop instantiations and tile classes a planes / blocked case runs"""
    sc = case_plan(c)
    blk = c.entry in ("blocked", "plan")
    tag = "wpb" if blk else "wp"
    out = {"balanced" if sc["balanced"] else "plain"}
    for cls in range(9):
        if not sc["T"][cls]:
            continue
        out.add("class-" + CLASS_NAMES[cls])
        wn, wk = planes_tile_widths(sc, cls)
        first_col = cls % 3 == 0 or sc["fK"] == 0 or (cls % 3 == 1 and sc["fK"] == 1)          # the class holds the tile at k0 == 0
        for wvn in (0, 1):
            for wvk in (0, 1):
                ni, nj = _wp_sub(wn, wvn, blk), _wp_sub(wk, wvk, blk)
                if ni == 0 or nj == 0:
                    out.add("idle-wave")
                    continue
                cs = c.cs and first_col and wvk == 0 and nj == 4
                out.add(f"{tag}<{_wp_round(ni)},{4 if cs else _wp_round(nj)}{',cs' if cs else ''}>")
                if first_col and wvk == 0 and nj != 4 and c.cs:
                    out.add("cs-without-instantiation")
    return out


# =====================================================================================================================================
# cases
# =====================================================================================================================================
# entry: f32 (usf_wgrad_f32) | bias (usf_wgrad_bias_f32) | jobs (a weight job of usf_grad_jobs_f32) | planes | blocked | plan
# (usf_wgrad_blocked_plan_f32 + usf_wgrad_reduce_jobs_f32).  kind: table | census (7 non-zero rows per Y column) | census4.
# pad: (ldy - N, lda - K, ldg - K) for fp32 operands; planes: (slack columns behind off + N, the same for A, ldg - K).
# off: (y_off, a_off) columns resp. (y_kb0, a_kb0) blocks.  kn: tuning knobs for the launch.
WCase = collections.namedtuple("WCase", "entry kind mode M N K alpha beta cs cs_ab pad off kn idx")
AB = [(1.0, 0.0), (0.5, -1.5), (-1.0, 1.0)]


def _w(entry, kind, mode, M, N, K, i, cs=False, off=(0, 0), kn=(), ab=None, pad=None):
    alpha, beta = ab or ((1.0, 0.0) if kind != "table" else AB[i % 3])
    cs_ab = ((1.0, 0.0) if kind != "table" else AB[(i + 1) % 3]) if cs else (0.0, 0.0)
    if pad is None:
        if entry in ("f32", "bias", "jobs"):
            pad = (ceil_to(N + 1 + i % 3, 4) - N, ceil_to(K + 2 + i % 5, 4) - K, 1 + i % 4)
        else:
            pad = (8 * (1 + i % 2), 8 * (1 + (i + 1) % 2), 1 + i % 4)
    return WCase(entry, kind, mode, M, N, K, alpha, beta, bool(cs), cs_ab, tuple(pad), tuple(off), tuple(kn), i)


F32_M = [0, 1, 15, 16, 17, 31, 32, 33, 256, 257, 601]
F32_NK = [1, 15, 16, 17, 48, 64, 65, 127, 128, 129, 144, 257]
BF_M = [2048, 2049, 2079, 2081]
LW_SHAPES = [(528, 544), (544, 528), (528, 528), (544, 544), (561, 593)]          # 4 x 128 + remainder: the nine (NI, NJ)
LW_SECOND = [(592, 608), (609, 577)]                                                 # remainders in 65 .. 127: the second wave row / column
EMPTY_NK = (528, 448)                                                                # 20 tiles: the fewest the loader-wave rule takes at 8192 rows
EMPTY_SMALL_NK = (128, 256)                                                          # 2 tiles: the 256-thread kernels' empty range
PL_M = [1, 31, 32, 33, 96, 97, 128, 129, 255, 288, 1001]
OFFS = [0, 8, 24]


def lw_last_range_Ms(N, K):
    """M from 8193 up whose last row range ends in a slab of ONE row and whose slab count takes each value mod 4"""
    out = {}
    for M in range(8193, 8193 + 32 * 64, 32):
        p = f32_plan(M, N, K, ceil_to(N, 4), ceil_to(K, 4), 1, False)
        b, e = plan_ranges(M, p["rows"], p["splits"])[-1]
        if p["variant"] == 2 and e - b > 0 and (e - b) % 32 == 1:
            out.setdefault(cdiv(e - b, 32) % 4, M)
        if len(out) == 4:
            break
    return [out[r] for r in sorted(out)]


def _build_f32_cases():
    cases, i = [], 0
    # mode 0: every M against a walk through the widths; every (ni, nj) of the edge path comes from the N x K grid below
    for j, M in enumerate(F32_M):
        for t in range(3):
            N, K = F32_NK[(5 * j + 7 * t) % 12], F32_NK[(3 * j + 5 * t + 4) % 12]
            cases.append(_w("f32", "table", 0, M, N, K, i)); i += 1
    for N, K in [(1, 17), (33, 49), (49, 1), (64, 33), (17, 64), (48, 48), (129, 33), (33, 257), (257, 257), (128, 128)]:
        cases.append(_w("f32", "table", 0, 33 + 224 * (i % 2), N, K, i)); i += 1
    for M, N, K in [(1, 17, 33), (33, 129, 65), (256, 48, 144), (257, 65, 129), (601, 144, 17)]:
        cases.append(_w("f32", "census", 0, M, N, K, i)); i += 1
    cases.append(_w("f32", "table", 0, 65537, *EMPTY_SMALL_NK, i)); i += 1          # an EMPTY last range (find_empty_range)
    # grad_jobs weight jobs
    for M, N, K in [(1, 17, 129), (32, 129, 48), (33, 65, 65), (256, 144, 257), (0, 16, 16)]:
        cases.append(_w("jobs", "table", 0, M, N, K, i)); i += 1
    cases.append(_w("jobs", "census", 0, 33, 65, 129, i)); i += 1
    # mode 1, 256 threads: ni, nj 1 .. 4 on both sides of the vector / scalar switch, column sums present and absent
    bf = [(2048, 16, 64), (2049, 31, 127), (2079, 48, 100), (2081, 64, 65), (2048, 130, 17), (2049, 161, 34), (2079, 177, 49),
          (2081, 257, 192), (2049, 15, 1), (2081, 100, 160)]
    for M, N, K in bf:
        cs = K >= 64
        cases.append(_w("bias" if cs else "f32", "table", 1, M, N, K, i, cs=cs)); i += 1
        cases.append(_w("bias" if cs else "f32", "census", 1, M, N, K, i, cs=cs)); i += 1
    cases.append(_w("f32", "table", 1, 2081, 100, 160, i)); i += 1
    cases.append(_w("f32", "census4", 1, 2079, 48, 100, i)); i += 1
    cases.append(_w("f32", "census", 1, 65537, *EMPTY_SMALL_NK, i)); i += 1
    # mode 1, loader waves
    for s, (N, K) in enumerate(LW_SHAPES + LW_SECOND):
        cs = s % 2 == 0 or s == 3
        M = 8193
        cases.append(_w("bias" if cs else "f32", "table", 1, M, N, K, i, cs=cs)); i += 1
        cases.append(_w("bias" if cs else "f32", "census", 1, M, N, K, i, cs=cs)); i += 1
    for M in lw_last_range_Ms(*LW_SHAPES[4])[1:]:
        cases.append(_w("f32", "census", 1, M, *LW_SHAPES[4], i)); i += 1
    cases.append(_w("f32", "table", 1, 8193, 544, 544, i)); i += 1
    cases.append(_w("f32", "census4", 1, 8225, 528, 544, i)); i += 1
    # wgrad_lw_min lowered: the smallest M the 160 000 row-tiles rule lets through at 25 tiles
    cases.append(_w("bias", "table", 1, 6401, 561, 593, i, cs=True, kn=(("wgrad_lw_min", 4096),))); i += 1
    M_empty = find_empty_range(*EMPTY_NK, 1, 8192, 70000)
    if M_empty:
        cases.append(_w("f32", "census", 1, M_empty, *EMPTY_NK, i)); i += 1
        cases.append(_w("f32", "table", 1, M_empty, *EMPTY_NK, i)); i += 1
    return cases


def _build_planes_cases():
    cases, i = [], 1000
    shapes = [  # (N, K): classes and instantiations by remainder -- see planes_instantiations
        (8, 8), (8, 17), (17, 16), (17, 40), (8, 64), (17, 65), (40, 8), (64, 17), (16, 144), (17, 144), (64, 145), (128, 144),
        (144, 136), (144, 145), (145, 129), (144, 64), (129, 128), (272, 273), (273, 272), (65, 272), (272, 65), (145, 16),
        (144, 8), (129, 17), (272, 144), (273, 129), (17, 17)]
    for j, (N, K) in enumerate(shapes):
        M = PL_M[(3 * j + 5) % 11] if j % 2 else PL_M[4 + (j // 2) % 7]          # odd j: any M; even j: M >= 96
        cs = K >= 64 and j % 3 != 2
        off = (OFFS[j % 3], OFFS[(j + 1) % 3])
        cases.append(_w("planes", "table", 1, M, N, K, i, cs=cs, off=off)); i += 1
    # every instantiation again on the balanced schedule with a census beside it (M >= 97), with and without column sums
    for j, (N, K) in enumerate(shapes):
        M = [97, 128, 129, 255, 288, 1001][j % 6]
        cs = K >= 64 and j % 2 == 0
        off = (OFFS[(j + 2) % 3], OFFS[j % 3])
        cases.append(_w("planes", "census" if j % 5 else "census4", 1, M, N, K, i, cs=cs, off=off)); i += 1
        if K >= 64:
            cases.append(_w("planes", "table", 1, M, N, K, i, cs=not cs, off=off)); i += 1
    # knobs: plain grid, no folding, one round; fN / fK = 0 and 1 with column sums (the reduction's tk0 rule)
    for kn, (M, N, K) in [((("wgrad_sched", 0),), (1001, 144, 144)), ((("wgrad_fold", 0),), (288, 144, 136)),
                          ((("wgrad_rounds", 1),), (1001, 272, 144)), ((("wgrad_sched", 0),), (129, 273, 65)),
                          ((("wgrad_rounds", 1),), (255, 129, 129)), ((("wgrad_fold", 0),), (1001, 129, 272))]:
        cases.append(_w("planes", "table", 1, M, N, K, i, cs=True, off=(8, 24), kn=kn)); i += 1
        cases.append(_w("planes", "census", 1, M, N, K, i, cs=True, off=(24, 0), kn=kn)); i += 1
    # ONE row range of 4 .. 9 slabs on the plain grid (the balanced schedule cuts these M into ranges of 1 .. 5 slabs), the last
    # slab one row long where M says so
    for j, M in enumerate([128, 129, 161, 193, 255, 288, 225]):
        N, K = [(144, 65), (17, 144), (65, 129)][j % 3]
        cases.append(_w("planes", "census", 1, M, N, K, i, cs=j % 2 == 0, off=(OFFS[j % 3], 8), kn=(("wgrad_sched", 0),))); i += 1
    # blocked operands: the 11 instantiations, kb0 > 0, a wide tile, edge tiles narrower than a block
    bshapes = [(8, 17), (40, 64), (17, 144), (144, 40), (64, 136), (144, 65), (129, 128), (272, 144), (65, 273), (100, 160), (160, 17),
               (273, 129)]
    for j, (N, K) in enumerate(bshapes):
        M = [97, 33, 128, 129, 255, 288, 1001, 17][j % 8]
        cs = K >= 64 and j % 2 == 0
        off = (j % 3, (j + 1) % 3)
        cases.append(_w("blocked", "table", 1, M, N, K, i, cs=cs, off=off)); i += 1
        cases.append(_w("blocked", "census", 1, max(M, 97), N, K, i, cs=K >= 64 and not cs, off=off)); i += 1
    return cases


F32_CASES = _build_f32_cases()
PLANES_CASES = _build_planes_cases()
# three gradients of different shape, reduced in ONE usf_wgrad_reduce_jobs_f32 launch
PLAN_CASES = [_w("plan", "table", 1, 129, 144, 136, 2000, cs=True, off=(1, 0)), _w("plan", "census", 1, 288, 65, 273, 2001, off=(0, 2)),
              _w("plan", "table", 1, 1001, 272, 64, 2002, cs=True, off=(2, 1))]
ALL_CASES = F32_CASES + PLANES_CASES + PLAN_CASES


def case_id(c):
    kn = "".join(f"-{k}{v}" for k, v in c.kn)
    return (f"{c.entry}-{c.kind}-m{c.mode}-M{c.M}-N{c.N}-K{c.K}-a{c.alpha:g}b{c.beta:g}{'-cs' if c.cs else ''}"
            f"-off{c.off[0]}_{c.off[1]}-pad{'_'.join(map(str, c.pad))}{kn}")


def case_lds(c):
    """(ldy, lda, ldg) of an fp32 case; planes: (ldyp, ldap, ldg)"""
    if c.entry in ("f32", "bias", "jobs"):
        return c.N + c.pad[0], c.K + c.pad[1], c.K + c.pad[2]
    if c.entry == "planes":
        return c.off[0] + ceil_to(c.N, 8) + c.pad[0], c.off[1] + ceil_to(c.K, 8) + c.pad[1], c.K + c.pad[2]
    return 0, 0, c.K + c.pad[2]


def case_nkb(c):
    """blocked: (y_nkb, a_nkb) -- one block of slack behind the operand's"""
    return c.off[0] + cdiv(c.N, 32) + 1, c.off[1] + cdiv(c.K, 32) + 1 + c.idx % 2


def case_workspace_floats(c, cus=CUS):
    if c.entry in ("f32", "bias"):
        return f32_workspace_floats(c.M, c.N, c.K)
    if c.entry == "jobs":
        return 0
    return planes_workspace_floats(c.M, c.N, c.K, cus, c.kn)


@functools.lru_cache(maxsize=None)
def case_plan(c, cus=CUS):
    if c.entry in ("f32", "bias"):
        ldy, lda, _ = case_lds(c)
        return f32_plan(c.M, c.N, c.K, ldy, lda, c.mode, c.cs, c.kn)
    if c.entry == "jobs":
        return dict(variant=0, splits=1, rows=ceil_to(c.M, 32) or 32, direct=1, grid=wg_tiles(c.N, c.K), threads=256, reduce=0, need=0)
    return planes_plan(c.M, c.N, c.K, case_workspace_floats(c, cus), cus, c.kn)


def case_ranges(c):
    """[(m_begin, m_end)] of the case's row ranges and the rows per slab"""
    p = case_plan(c)
    if c.entry in ("f32", "bias", "jobs"):
        return plan_ranges(c.M, p["rows"], p["splits"]), (32 if p["variant"] else 16)
    rows = max(p["rows"])
    return plan_ranges(c.M, rows, p["parts"]), 32


def case_instantiations(c):
    return f32_instantiations(c) if c.entry in ("f32", "bias", "jobs") else planes_instantiations(c)


def case_label(c):
    """the print line's instantiation column"""
    inst = sorted(x for x in case_instantiations(c) if "<" in x or x in ("f32-full", "empty-range"))
    return "+".join(inst) or "none"


# =====================================================================================================================================
# operands
# =====================================================================================================================================
def risk_rows(c):
    """rows where the pipeline is at risk: first and last row of every row range, row M - 1, one row in each of the first three
    slabs of the first and of the last range (the ring's slots) and the first row of every range's last slab (the slab in front
    of a surplus iteration)"""
    ranges, slab = case_ranges(c)
    rows = []
    live = [(b, e) for b, e in ranges if b < e]
    for b, e in live:
        rows += [b, e - 1, b + (cdiv(e - b, slab) - 1) * slab]
    for b, e in (live[:1] + live[-1:]):
        rows += [min(b + s * slab + 5, e - 1) for s in range(3)]
    rows.append(c.M - 1)
    return sorted(set(r for r in rows if 0 <= r < c.M))


def census_rows(c):
    """[nz, N] row indices: the non-zero rows of every Y column, walking through risk_rows"""
    nz = min(4 if c.kind == "census4" else 7, c.M)
    risk = risk_rows(c)
    pool = risk + [r for r in range(min(c.M, 64)) if r not in set(risk)]
    L = len(pool)
    assert L >= nz
    n = torch.arange(c.N)
    return torch.stack([torch.tensor(pool)[(n * nz + t) % L] for t in range(nz)])


def _census_values(shape, g):
    s = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    a = torch.randint(1, 4, shape, generator=g).double()
    b = torch.randint(1, 4, shape, generator=g).double()
    return (s * (1 + a * 2.0 ** -10 + b * 2.0 ** -20)).float()


def _values(c, perm_seed=0):
    """(Y [M, N], A [M, K]) fp32"""
    g = torch.Generator().manual_seed(_seed(c.idx, c.M, c.N, c.K, perm_seed))
    M, N, K = c.M, c.N, c.K
    if c.kind == "table":
        return torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    if c.mode == 0:          # small integers: every product and every sum exact in fp32
        return torch.randint(-3, 4, (M, N), generator=g).float(), torch.randint(-3, 4, (M, K), generator=g).float()
    Y = torch.zeros(M, N)
    rows = census_rows(c)
    Y[rows, torch.arange(N).expand_as(rows)] = _census_values(rows.shape, g)
    return Y, _census_values((M, K), g)


def _fp32_buffer(vals, rows_total, ld, salt):
    """[guard | rows_total x ld, NaN but vals in the top left | guard] flat; the buffer's address is GF floats in"""
    M, N = vals.shape
    body = nan_f32(rows_total * ld, salt).clone().view(rows_total, ld)
    body[:M, :N] = vals
    return torch.cat([nan_f32(GF, salt + 1), body.reshape(-1), nan_f32(GF, salt + 2)])


def _planes_rowmajor(vals, off, ld, gap, salt):
    """row-major planes [3][ceil32(M)][ld] + `gap` elements between planes as int16 bits with guards; NaN outside [off, off + N),
    zeros in rows [M, ceil32(M))"""
    M, N = vals.shape
    R = ceil_to(M, 32)
    stride = R * ld + gap
    flat = nan_bits16(3 * stride, 3, salt).clone()
    pl = split_planes(vals.contiguous(), 3)
    for q in range(3):
        v = flat[q * stride: q * stride + R * ld].view(R, ld)
        v[:M, off: off + N] = bits16(pl[q])
        v[M:] = 0
    return torch.cat([nan_bits16(GH, 3, salt + 1), flat, nan_bits16(GH, 3, salt + 2)]), stride


def _planes_blocked(vals, kb0, nkb, zero_pad_rows, salt):
    """a blocked planes buffer (include/usflows_hip.h) of ceil(M / 16) panels x nkb blocks as int16 bits with guards: NaN in every
    block outside the operand's and in the positions >= N of its last block; padding rows zero (Y) or finite junk (A)"""
    M, N = vals.shape
    R = ceil_to(M, 16)
    bits = nan_bits16(3 * R * 32 * nkb, 3, salt).view(3, R, 32 * nkb).clone()
    bits[:, :M, 32 * kb0: 32 * kb0 + N] = bits16(split_planes(vals.contiguous(), 3))
    live = slice(32 * kb0, 32 * (kb0 + cdiv(N, 32)))
    if zero_pad_rows:
        bits[:, M:, live] = 0
    else:
        g = torch.Generator().manual_seed(_seed(salt, 5))
        junk = torch.randn(3, R - M, live.stop - live.start, generator=g) * 100
        bits[:, M:, live] = bits16(junk.to(torch.bfloat16))
    return torch.cat([nan_bits16(GH, 3, salt + 1), to_chunks(bits), nan_bits16(GH, 3, salt + 2)])


INPUTS = ("Y", "A")


@functools.lru_cache(maxsize=6)
def prepared(c):
    """buffers and references of a case.  Y / A: flat guarded input buffers; G0, cs0, ws0: the output buffers before the launch."""
    M, N, K = c.M, c.N, c.K
    Yv, Av = _values(c)
    ldy, lda, ldg = case_lds(c)
    g = torch.Generator().manual_seed(_seed(c.idx, 77))
    p = dict(Yv=Yv, Av=Av, ldy=ldy, lda=lda, ldg=ldg)
    if c.entry in ("f32", "bias", "jobs"):
        p["Y"] = _fp32_buffer(Yv, M + EXTRA_ROWS, ldy, 3 * c.idx)
        p["A"] = _fp32_buffer(Av, M + EXTRA_ROWS, lda, 3 * c.idx + 1)
    elif c.entry == "planes":
        p["Y"], p["ystride"] = _planes_rowmajor(Yv, c.off[0], ldy, 8 * (c.idx % 3), 3 * c.idx)
        p["A"], p["astride"] = _planes_rowmajor(Av, c.off[1], lda, 8 * ((c.idx + 1) % 3), 3 * c.idx + 1)
    else:
        y_nkb, a_nkb = case_nkb(c)
        p["Y"] = _planes_blocked(Yv, c.off[0], y_nkb, True, 3 * c.idx)
        p["A"] = _planes_blocked(Av, c.off[1], a_nkb, False, 3 * c.idx + 1)
    # G: [guard | (N + 2) x ldg | guard]; the live part holds NaN where beta == 0
    Gb = nan_f32((N + 2) * ldg, 3 * c.idx + 2).clone().view(N + 2, ldg)
    if c.beta != 0:
        Gb[:N, :K] = torch.randn(N, K, generator=g)
    p["G0"] = torch.cat([nan_f32(GF, c.idx + 5), Gb.reshape(-1), nan_f32(GF, c.idx + 6)])
    csb = nan_f32(N + 5, c.idx + 7).clone()
    if c.cs and c.cs_ab[1] != 0:
        csb[:N] = torch.randn(N, generator=g)
    p["cs0"] = torch.cat([nan_f32(GF, c.idx + 8), csb, nan_f32(GF, c.idx + 9)])
    p["ws0"] = nan_f32(case_workspace_floats(c) + GF, c.idx + 10).clone()
    p.update(_references(c, p))
    return p


def g_view(c, flat, ldg):
    return flat[GF: flat.numel() - GF].view(c.N + 2, ldg)


def _ranges_fp32(Y, A, ranges, slab):
    """[ranges][N, K] partial sums in fp32, slab by slab"""
    parts = []
    for b, e in ranges:
        acc = torch.zeros(Y.shape[1], A.shape[1])
        for m in range(b, e, slab):
            acc += Y[m: min(m + slab, e)].t() @ A[m: min(m + slab, e)]
        parts.append(acc)
    return parts


def _finish32(parts, alpha, beta, old):
    s = torch.zeros_like(parts[0])
    for q in parts:
        s = s + q
    v = alpha * s
    return v + beta * old if beta != 0 else v


def _references(c, p):
    Y, A, N, K = p["Yv"], p["Av"], c.N, c.K
    ranges, slab = case_ranges(c)
    G0 = g_view(c, p["G0"], p["ldg"])[:N, :K]
    cs0 = p["cs0"][GF: GF + N]
    r = {}
    prod = Y.double().t() @ A.double() if c.M else torch.zeros(N, K, dtype=torch.float64)
    r["ref"] = c.alpha * prod + (c.beta * G0.double() if c.beta != 0 else 0)
    r["f32"] = _finish32(_ranges_fp32(Y, A, ranges, slab), c.alpha, c.beta, G0)
    if c.cs:
        ca, cb = c.cs_ab
        r["cs_ref"] = ca * Y.double().sum(0) + (cb * cs0.double() if cb != 0 else 0)
        ones = torch.ones(c.M, 1)
        r["cs_f32"] = _finish32([q[:, 0] for q in _ranges_fp32(Y, ones, ranges, slab)], ca, cb, cs0)
    if c.kind != "table":
        r["census"] = census_expected(c, p)
    return r


def census_expected(c, p, products=KEPT, ranges=None, extra_rows=None):
    """the sum of `products` over the rows of `ranges` (default: all rows once) in fp64 -- exact for census operands"""
    Y, A = p["Yv"], p["Av"]
    if c.mode == 0:
        Yp, Ap, products = [Y.double()], [A.double()], [(0, 0)]
    else:
        Yp, Ap = [q.double() for q in split_planes(Y, 3)], [q.double() for q in split_planes(A, 3)]
    idx = torch.arange(c.M) if ranges is None else torch.cat([torch.arange(b, e) for b, e in ranges] + [torch.arange(0)])
    if extra_rows is not None:
        idx = torch.cat([idx, extra_rows])
    out = torch.zeros(c.N, c.K, dtype=torch.float64)
    by_y = collections.defaultdict(list)
    for i, j in products:
        by_y[i].append(j)
    for i, js in by_y.items():
        a = Ap[js[0]][idx].clone()
        for j in js[1:]:
            a += Ap[j][idx]
        out += Yp[i][idx].t() @ a
    return out


def census_orders(c, p):
    """the six kept products of a bf16x3 census case summed in fp32 in three orders (row-major, product-major, reversed): three
    [N, K] fp32 results, for the CPU test's exactness claim"""
    Yp, Ap = split_planes(p["Yv"], 3).float(), split_planes(p["Av"], 3).float()
    rows = census_rows(c)
    cols = torch.arange(c.N)
    terms = [(Yp[i][rows[t], cols][:, None], Ap[j][rows[t]]) for t in range(rows.shape[0]) for i, j in KEPT]
    by_product = [terms[t * 6 + q] for q in range(6) for t in range(rows.shape[0])]
    outs = []
    for order in (terms, by_product, terms[::-1]):
        acc = torch.zeros(c.N, c.K)
        for y, a in order:
            acc = acc + y * a          # fp32 product, fp32 sum
        outs.append(acc)
    return outs


# =====================================================================================================================================
# checks
# =====================================================================================================================================
def check(c, got, p):
    """got: dict(G, cs, ws) of flat buffers after the launch.  Returns ([failures "name: detail"], figures)"""
    N, K, ldg = c.N, c.K, p["ldg"]
    bad = []
    G = g_view(c, got["G"], ldg)
    live = G[:N, :K]
    # 3. everything else as it was
    mask = torch.ones(got["G"].numel(), dtype=torch.bool)
    mask[GF: -GF].view(N + 2, ldg)[:N, :K] = False
    if not torch.equal(bits32(got["G"])[mask], bits32(p["G0"])[mask]):
        where = (bits32(got["G"]) != bits32(p["G0"])) & mask
        bad.append(f"guard: G changed outside [N, K] at flat {where.nonzero()[:4].flatten().tolist()}")
    csm = torch.ones(got["cs"].numel(), dtype=torch.bool)
    if c.cs:
        csm[GF: GF + N] = False
    if not torch.equal(bits32(got["cs"])[csm], bits32(p["cs0"])[csm]):
        bad.append("guard: colsum_out changed beyond N")
    nws = p["ws0"].numel() - GF
    if not torch.equal(bits32(got["ws"])[nws:], bits32(p["ws0"])[nws:]):
        bad.append("guard: the workspace's guard changed")
    if torch.isnan(live).any():
        bad.append(f"nan: {int(torch.isnan(live).sum())} NaN in G")
    cs = got["cs"][GF: GF + N]
    if c.cs and torch.isnan(cs).any():
        bad.append(f"nan: {int(torch.isnan(cs).sum())} NaN in the column sums")
    # 1. parity
    fig = {}
    for name, val, ref, f32 in [("G", live, p["ref"], p["f32"])] + ([("cs", cs, p["cs_ref"], p["cs_f32"])] if c.cs else []):
        mag = float(ref.abs().max()) or 1.0
        err = float((val.double() - ref).abs().max()) / mag
        err32 = float((f32.double() - ref).abs().max()) / mag
        bound = max(4 * err32, 6e-8 * math.sqrt(max(c.M, 1)))
        fig[name] = dict(err=err, err32=err32, bound=bound)
        if not err <= bound:
            bad.append(f"parity: {name} err {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})")
    # 2. census
    if c.kind != "table":
        exp = (c.alpha * p["census"]).float()
        if not torch.equal(bits32(live), bits32(exp)):
            d = (live.double() - exp.double())
            nz = d != 0
            bad.append(f"census: {int(nz.sum())} of {nz.numel()} elements differ, by {sorted(set((d[nz] * 2.0 ** 30).round().tolist()))[:8]} x 2^-30")
        if c.cs and not torch.equal(bits32(cs), bits32(p["Yv"].double().sum(0).float())):
            bad.append("census: the column sums differ from the exact sums")
    fig["census"] = "-" if c.kind == "table" else ("exact" if not any(b.startswith("census") for b in bad) else "DIFFERS")
    return bad, fig


def report_line(c, fig):
    f = fig["G"]
    cs = f"|cs {fig['cs']['err']:.3e}/{fig['cs']['err32']:.3e}/{fig['cs']['bound']:.3e}" if "cs" in fig else "|"
    return (f"WK|{c.entry}|{case_label(c)}|{c.kind}|M{c.M} N{c.N} K{c.K}|{f['err']:.3e}|{f['err32']:.3e}|{f['bound']:.3e}{cs}"
            f"|{fig['census']}")


# =====================================================================================================================================
# the CPU stand-in for a launch, and its mutants
# =====================================================================================================================================
MUTANTS = ["drop_Y2A0", "drop_Y1A1", "drop_Y0A2", "dup_Y1A0", "last_row_of_range", "second_range_first_slab_twice", "partial_left_out",
           "class_count_from_other_class", "dead_subtile_stored", "store_past_K", "colsum_from_tile_column_1", "beta_where_zero",
           "nan_from_padding_column", "extension_swapped", "blk_pos_identity", "row_ge_M"]


def wp_blk_pos(c, tt):
    return 16 * (((c >> 2) & 1) ^ tt) + 4 * (c >> 2) + (c & 3)


def emulate(c, p, mutant=None):
    """what a correct launch leaves behind (census: the exact sums; table: the fp32 restatement), or what `mutant` would"""
    N, K, M, ldg = c.N, c.K, c.M, p["ldg"]
    Gf, csf, ws = p["G0"].clone(), p["cs0"].clone(), p["ws0"].clone()
    G = g_view(c, Gf, ldg)
    ranges, slab = case_ranges(c)
    G0 = G[:N, :K].clone()

    def fin(s, old, a, b):
        v = a * s.float()
        return v + b * old if b != 0 else v

    census = c.kind != "table"
    products = list(KEPT)
    if mutant and mutant.startswith("drop_"):
        products.remove({"drop_Y2A0": (2, 0), "drop_Y1A1": (1, 1), "drop_Y0A2": (0, 2)}[mutant])
    if mutant == "dup_Y1A0":
        products[products.index((0, 1))] = (1, 0)
    rg, extra = None, None
    live = [(b, e) for b, e in ranges if b < e]
    if mutant == "last_row_of_range":
        rg = [(b, e - 1) if k == 0 else (b, e) for k, (b, e) in enumerate(live)]
    if mutant == "second_range_first_slab_twice":
        b, e = live[1]
        rg, extra = live, torch.arange(b, min(b + slab, e))
    if mutant in ("partial_left_out", "class_count_from_other_class"):
        rg = live[:-1]
    if census:
        s = census_expected(c, p, products, rg, extra)
    else:
        s = _finish32(_ranges_fp32(p["Yv"], p["Av"], rg or ranges, slab), 1.0, 0.0, None).double()
    if mutant == "class_count_from_other_class":
        # the tiles of the first tile class keep their own count; every other class loses its last partial
        full = census_expected(c, p, products) if census else _finish32(_ranges_fp32(p["Yv"], p["Av"], ranges, slab), 1.0, 0.0, None).double()
        full[128 * case_plan(c)["fN"]:, :] = s[128 * case_plan(c)["fN"]:, :]
        s = full
    if mutant == "extension_swapped":
        k0 = 128 * (case_plan(c)["fK"] - 1)
        s = s.clone()
        s[:, k0: k0 + 16], s[:, k0 + 128: k0 + 144] = s[:, k0 + 128: k0 + 144].clone(), s[:, k0: k0 + 16].clone()
    if mutant == "blk_pos_identity":
        perm = torch.tensor([32 * (k // 32) + wp_blk_pos(k % 16, (k % 32) // 16) for k in range(ceil_to(K, 32))])
        s = torch.cat([s, torch.zeros(N, ceil_to(K, 32) - K, dtype=s.dtype)], 1)[:, perm][:, :K]
    if mutant == "row_ge_M":
        Yb, Ab = p["Y"][GF:-GF].view(M + EXTRA_ROWS, p["ldy"]), p["A"][GF:-GF].view(M + EXTRA_ROWS, p["lda"])
        s = s + Yb[M, :N, None].double() * Ab[M, None, :K].double()
    if mutant == "nan_from_padding_column":
        Yb = p["Y"][GF:-GF].view(M + EXTRA_ROWS, p["ldy"])
        s = s.clone()
        s[N - 1] += Yb[:M, N].double() @ p["Av"].double()
    beta = c.beta if mutant != "beta_where_zero" else (c.beta or 1.0)
    G[:N, :K] = fin(s, G0, c.alpha, beta)
    if mutant == "dead_subtile_stored":
        G[N: N + 1, :K] = 0.0
    if mutant == "store_past_K":
        G[:N, K] = G[:N, K - 1]
    if c.cs:
        ca, cb = c.cs_ab
        if census:
            t = p["Yv"].double().sum(0)
        else:
            t = _finish32([q[:, 0] for q in _ranges_fp32(p["Yv"], torch.ones(M, 1), ranges, slab)], 1.0, 0.0, None).double()
        if mutant == "colsum_from_tile_column_1" and K <= 128:
            t = ws[:N].double()          # nobody wrote the partial column sums: the workspace's NaN
        csf[GF: GF + N] = fin(t, csf[GF: GF + N].clone(), ca, cb)
    return dict(G=Gf, cs=csf, ws=ws)


# =====================================================================================================================================
# usf_colsum_f32 and the column-sum jobs of usf_grad_jobs_f32
# =====================================================================================================================================
CCase = collections.namedtuple("CCase", "entry kind M N pad alpha beta idx")
COLSUM_CASES = (
    [CCase("colsum", "table", M, N, 1 + (i % 3), *AB[i % 3], 3000 + i)
     for i, (M, N) in enumerate([(0, 1), (1, 63), (17, 64), (256, 65), (257, 1), (65536, 63), (65537, 8), (257, 64), (65537, 5)])]
    + [CCase("colsum", "census", M, N, 2, 1.0, 0.0, 3020 + i) for i, (M, N) in enumerate([(17, 65), (257, 63), (65537, 7)])]
    + [CCase("jobcs", "table", M, N, 1 + (i % 3), *AB[i % 3], 3040 + i)
       for i, (M, N) in enumerate([(1, 1), (33, 63), (255, 64), (17, 65), (31, 130), (3, 64)])]
    + [CCase("jobcs", "census", 33, 130, 3, 1.0, 0.0, 3060)])


def ccase_id(c):
    return f"{c.entry}-{c.kind}-M{c.M}-N{c.N}-ld{c.N + c.pad}-a{c.alpha:g}b{c.beta:g}"


def colsum_levels(M):
    """kernel launches of usf_colsum_f32: 256-row levels until one range is left"""
    n, rows = 1, M
    while cdiv(rows, 256) > 1:
        rows = cdiv(rows, 256)
        n += 1
    return n


def colsum_workspace_floats(M, N):
    return (cdiv(M, 256) + cdiv(M, 65536) + 2) * N


def _colsum_level32(X, lanes):
    """colsum_kernel / grad_jobs_kernel's order in fp32: `lanes` row lanes walk a range of 256 rows (colsum) resp. all rows (jobs),
    the lanes are added in order"""
    R, N = X.shape
    span = 256 if lanes == 16 else max(ceil_to(R, lanes), lanes)
    nb = max(cdiv(R, span), 1)
    Xp = torch.zeros(nb * span, N)
    Xp[:R] = X
    Xp = Xp.view(nb, span // lanes, lanes, N)
    s = torch.zeros(nb, lanes, N)
    for step in range(span // lanes):
        s = s + Xp[:, step]
    t = torch.zeros(nb, N)
    for lane in range(lanes):
        t = t + s[:, lane]
    return t


def colsum32(c, X):
    if c.entry == "jobcs":
        return _colsum_level32(X, 4)[0]
    t = _colsum_level32(X, 16)
    while t.shape[0] > 1:
        t = _colsum_level32(t, 16)
    return t[0]


@functools.lru_cache(maxsize=4)
def colsum_prepared(c):
    g = torch.Generator().manual_seed(_seed(c.idx, c.M, c.N))
    M, N, ld = c.M, c.N, c.N + c.pad
    Yv = torch.randn(M, N, generator=g) if c.kind == "table" else torch.randint(-3, 4, (M, N), generator=g).float()
    out = nan_f32(N + 5, c.idx).clone()
    if c.beta != 0:
        out[:N] = torch.randn(N, generator=g)
    p = dict(Yv=Yv, ld=ld, Y=_fp32_buffer(Yv, M + EXTRA_ROWS, ld, c.idx + 1),
             out0=torch.cat([nan_f32(GF, c.idx + 2), out, nan_f32(GF, c.idx + 3)]),
             ws0=nan_f32(colsum_workspace_floats(M, N) + GF, c.idx + 4).clone())
    old = out[:N]
    p["ref"] = c.alpha * Yv.double().sum(0) + (c.beta * old.double() if c.beta != 0 else 0)
    t = c.alpha * colsum32(c, Yv)
    p["f32"] = t + c.beta * old if c.beta != 0 else t
    return p


def colsum_check(c, got, p):
    N, bad = c.N, []
    mask = torch.ones(got["out"].numel(), dtype=torch.bool)
    mask[GF: GF + N] = False
    if not torch.equal(bits32(got["out"])[mask], bits32(p["out0"])[mask]):
        bad.append("guard: out changed beyond N")
    nws = p["ws0"].numel() - GF
    if not torch.equal(bits32(got["ws"])[nws:], bits32(p["ws0"])[nws:]):
        bad.append("guard: the workspace's guard changed")
    v = got["out"][GF: GF + N]
    if torch.isnan(v).any():
        bad.append("nan: NaN in the column sums")
    mag = float(p["ref"].abs().max()) or 1.0
    err = float((v.double() - p["ref"]).abs().max()) / mag
    err32 = float((p["f32"].double() - p["ref"]).abs().max()) / mag
    bound = max(4 * err32, 6e-8 * math.sqrt(max(c.M, 1)))
    if not err <= bound:
        bad.append(f"parity: err {err:.3e} > bound {bound:.3e} (err32 {err32:.3e})")
    if c.kind == "census" and not torch.equal(bits32(v), bits32(p["ref"].float())):
        bad.append("census: the column sums of small integers differ from the exact sums")
    return bad, dict(err=err, err32=err32, bound=bound, census="-" if c.kind == "table" else ("exact" if not bad else "DIFFERS"))


def colsum_emulate(c, p, mutant=None):
    out, ws = p["out0"].clone(), p["ws0"].clone()
    t = colsum32(c, p["Yv"]) if c.kind == "table" else p["Yv"].double().sum(0).float()
    if mutant == "row_ge_M":
        t = t + p["Y"][GF:-GF].view(c.M + EXTRA_ROWS, p["ld"])[c.M, :c.N]
    if mutant == "last_row_of_range":
        t = t - p["Yv"][c.M - 1]
    beta = c.beta if mutant != "beta_where_zero" else (c.beta or 1.0)
    old = out[GF: GF + c.N].clone()
    out[GF: GF + c.N] = c.alpha * t + (beta * old if beta != 0 else 0)
    if mutant == "store_past_K":
        out[GF + c.N] = 0.0
    return dict(out=out, ws=ws)


# =====================================================================================================================================
# usf_split_planes_f32
# =====================================================================================================================================
SCase = collections.namedtuple("SCase", "path M N ldx ldp gap idx")          # path: vec | ldx_odd | misaligned | sweep_vec | sweep_scalar
SWEEP_PATTERNS = [0x000000, 0x7FFFFF, 0x400001, 0x2AAAAA, 0x555555, 0x7F807F, 0x00FF01, 0x123457]          # mantissa bits
SWEEP_N = 2 * len(SWEEP_PATTERNS)
# the exponents (of 2, of a NORMAL fp32 value 1.m x 2^e) on which every swept value is the exact sum of its three planes:
# below, the third plane's bits fall under bf16's smallest subnormal 2^-133; at 127 a mantissa above 1.fe rounds the first plane to infinity
SPLIT_EXACT_EMIN, SPLIT_EXACT_EMAX = -110, 126
SPLIT_CASES = (
    [SCase(path, M, N, ldx, ceil_to(N, 8) + 8 * (i % 2), 8 * (i % 3), 4000 + i)
     for i, (path, M, N, ldx) in enumerate([("vec", 1, 12, 12), ("vec", 33, 21, 24), ("ldx_odd", 31, 13, 13), ("ldx_odd", 32, 27, 29),
                                            ("misaligned", 33, 20, 24), ("misaligned", 1, 9, 12), ("ldx_odd", 33, 8, 9),
                                            ("misaligned", 31, 17, 20), ("vec", 32, 8, 8)])]
    + [SCase("sweep_vec", 277, SWEEP_N, SWEEP_N, SWEEP_N, 0, 4100), SCase("sweep_scalar", 277, SWEEP_N, SWEEP_N + 1, SWEEP_N + 8, 8, 4101)])


def scase_id(c):
    return f"{c.path}-M{c.M}-N{c.N}-ldx{c.ldx}-ldp{c.ldp}-gap{c.gap}"


def split_is_vector(c):
    """split_planes_kernel's `vec`: a 16-byte aligned base and ldx % 4 == 0"""
    return c.path in ("vec", "sweep_vec") and c.ldx % 4 == 0


def sweep_values():
    """[277, 16]: row r = biased exponent r (0: subnormals, 255 left out) for r < 255, the mantissas of SWEEP_PATTERNS in both
    signs; the rows from 255 hold zeros, negative zeros and the largest / smallest values"""
    e = torch.arange(277, dtype=torch.int64).clamp(max=254)[:, None]
    m = torch.tensor(SWEEP_PATTERNS, dtype=torch.int64)[None, :]
    pos = (e << 23) | m
    bits = torch.cat([pos, pos | 0x80000000], 1)
    bits[255:] = torch.tensor([0, 0x80000000, 1, 0x80000001, 0x7F7FFFFF, 0x007FFFFF, 0x00800000, 0x3F800000] * 2)
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def split_prepared(c):
    g = torch.Generator().manual_seed(_seed(c.idx))
    Xv = sweep_values() if c.path.startswith("sweep") else torch.randn(c.M, c.N, generator=g) * torch.exp2(
        torch.randint(-20, 20, (c.M, c.N), generator=g).float())
    body = nan_f32((c.M + EXTRA_ROWS) * c.ldx, c.idx).clone().view(-1, c.ldx)
    body[:c.M, :c.N] = Xv
    lead = GF + (1 if c.path == "misaligned" else 0)          # a base 4 bytes off 16-byte alignment
    X = torch.cat([nan_f32(lead, c.idx + 1), body.reshape(-1), nan_f32(GF, c.idx + 2)])
    R = ceil_to(c.M, 32)
    stride = R * c.ldp + c.gap
    P0 = torch.cat([nan_bits16(GH, 3, c.idx), nan_bits16(3 * stride, 3, c.idx + 1), nan_bits16(GH, 3, c.idx + 2)]).clone()
    exp = P0.clone()
    pl = bits16(split_planes(Xv.contiguous(), 3))
    for q in range(3):
        v = exp[GH + q * stride: GH + q * stride + R * c.ldp].view(R, c.ldp)
        v[:] = 0
        v[:c.M, :c.N] = pl[q]
    # where the first plane overflows (|x| above bf16's largest value) the later planes are inf - inf: a NaN, any payload
    any_nan = torch.zeros(exp.numel(), dtype=torch.bool)
    for q in range(3):
        any_nan[GH + q * stride: GH + q * stride + R * c.ldp].view(R, c.ldp)[:c.M, :c.N] = torch.isnan(pl[q].view(torch.bfloat16).float())
    return dict(Xv=Xv, X=X, x_off=lead, P0=P0, expected=exp, stride=stride, any_nan=any_nan)


def split_exact_rows(planes_bits, Xv):
    """per row of Xv: is every value the exact sum (p0 + p1) + p2 of its planes, in fp64"""
    s = planes_bits.view(torch.bfloat16).double().sum(0)
    return ((s == Xv.double()) | (torch.isnan(s) & torch.isnan(Xv.double()))).all(1)


def split_exact_exponents(exact_rows):
    """(emin, emax): the widest run of unbiased exponents of normal values around 0 whose sweep rows are all exact"""
    ok = [bool(exact_rows[r]) for r in range(255)]
    lo = hi = 127
    while lo - 1 >= 1 and ok[lo - 1]:
        lo -= 1
    while hi + 1 <= 254 and ok[hi + 1]:
        hi += 1
    return lo - 127, hi - 127


def split_check(c, got, p):
    bad = []
    same = (got == p["expected"]) | (p["any_nan"] & torch.isnan(got.view(torch.bfloat16).float()))
    if not bool(same.all()):
        d = (~same).nonzero().flatten()
        bad.append(f"bits: {d.numel()} plane elements differ from the round-to-nearest split (first at {d[:4].tolist()})")
    return bad

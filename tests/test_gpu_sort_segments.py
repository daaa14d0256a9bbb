"""The segmented radix sort of the batched front end (prims.hip: ghicp_sort_segments; tiles, chunks and digit places: csrc/sort_plan.h) against
numpy's stable argsort segment by segment, and the batched front end that runs on it against the cloud-by-cloud one.  Integer work with an
exact answer: every comparison is assert_array_equal.  The outputs are windows of larger device tensors full of guard words; every word outside
the window must still be the guard afterwards, and the inputs must be untouched.

Shapes, with T = 4096 the sort's tile: one segment of 1, T - 1, T, T + 1, 2 T + 1 keys; segments that end on a tile edge and one key either side;
empty segments first, in the middle and last; 33 and 64 segments (which needed 6 id bits in the one sort over id and key), with every segment
inside one tile (one launch for all places) and with one beyond it (the tiled launches); a segment beyond 64 tiles (the chunked scan).
Keys: all equal; the top bit of the top place; bit counts that are a multiple of the digit width and one more; segments of different bit
counts; cell keys above a per-segment base.  Both digit widths (8: places of 8 bits only; 9)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 4096
GUARD_WORDS = 64
GUARD = np.int32(-1515870811)  # 0xA5A5A5A5
U32, U64 = np.uint32, np.uint64


def framed(ctx, n_words):
    t = ctx.torch
    buf = t.full((2 * GUARD_WORDS + n_words + 2,), int(GUARD), dtype=t.int32, device=ctx.dev)
    lead = GUARD_WORDS + (buf.data_ptr() // 4 + GUARD_WORDS) % 2  # 8-byte aligned window
    return buf, buf[lead:lead + n_words], lead


def guards_intact(buf, lead, written):
    b = buf.cpu().numpy()
    return bool((b[:lead] == GUARD).all() and (b[lead + written:] == GUARD).all())


def seg_ref(k, sizes, bases, b, bits):
    """the permutation of a stable sort of every segment on the bits [b, b + bits) of key - base"""
    order, at = [], 0
    for s, n in enumerate(sizes):
        sub = ((k[at:at + n].astype(U64) - U64(bases[s] if bases is not None else 0)) >> U64(b)) & U64((1 << bits) - 1)
        order.append(at + np.argsort(sub, kind="stable"))
        at += n
    return np.concatenate(order) if order else np.zeros(0, np.int64)


def check(ctx, k, sizes, b, bits, with_vals, width, bases=None, what=""):
    t = ctx.torch
    n = int(sum(sizes))
    assert k.shape[0] == n
    kb = k.dtype.itemsize
    ks = k.view(np.int32 if kb == 4 else np.int64)
    kd = t.from_numpy(ks.copy()).to(ctx.dev)
    kbuf, kwin, klead = framed(ctx, n * (kb // 4))
    v = np.arange(n, dtype=np.int32)[::-1].copy() if with_vals else None
    vd = t.from_numpy(v.copy()).to(ctx.dev) if with_vals else None
    vbuf, vwin, vlead = framed(ctx, n) if with_vals else (None, None, 0)
    off = (ctypes.c_int64 * (len(sizes) + 1))(*np.r_[0, np.cumsum(sizes)].astype(np.int64).tolist())
    bd = t.from_numpy(np.asarray(bases, U32).view(np.int32).copy()).to(ctx.dev) if bases is not None else None
    ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    rc = ctx.lib.ghicp_sort_segments(ctx.h, ctypes.c_int(kb), ptr(kd), ptr(kwin), ptr(vd), ptr(vwin), ctypes.c_int32(len(sizes)), off, ptr(bd),
                                     ctypes.c_int(b), ctypes.c_int(bits), ctypes.c_int(width))
    assert rc == 0, (what, ctx.lib.ghicp_last_error(ctx.h))
    order = seg_ref(k, sizes, bases, b, bits)
    tag = "%s sizes=%s bits=[%d,+%d) width=%d kb=%d vals=%s" % (what, list(sizes)[:8], b, bits, width, kb, with_vals)
    got = kwin.cpu().numpy() if kb == 4 else kwin.view(t.int64).cpu().numpy()
    np.testing.assert_array_equal(got, ks[order], err_msg=tag + " (keys)")
    np.testing.assert_array_equal(kd.cpu().numpy(), ks, err_msg=tag + " (keys in)")
    assert guards_intact(kbuf, klead, n * (kb // 4)), tag
    if with_vals:
        np.testing.assert_array_equal(vwin.cpu().numpy(), v[order], err_msg=tag + " (values)")
        np.testing.assert_array_equal(vd.cpu().numpy(), v, err_msg=tag + " (values in)")
        assert guards_intact(vbuf, vlead, n), tag


def packed(rng, n, key_bits, idx_bits, seg_id=0, id_shift=None):
    """8-byte keys as the voxel filter packs them: (id above the key bits, key) << idx_bits | index"""
    key = rng.integers(0, 1 << key_bits, n, dtype=np.uint64) if key_bits else np.zeros(n, U64)
    if id_shift is not None:
        key |= U64(seg_id) << U64(id_shift)
    return (key << U64(idx_bits)) | np.arange(n, dtype=U64)


def both_kinds(ctx, rng, sizes, bits, width, what):
    """the front end's two uses: packed 8-byte keys without values on bits above the index; 4-byte cell keys with values above a segment base"""
    n = int(sum(sizes))
    idx_bits = max(1, int(n - 1).bit_length())
    k8 = np.concatenate([packed(rng, m, bits, idx_bits, s, bits) + U64(sum(sizes[:s])) for s, m in enumerate(sizes)] + [np.zeros(0, U64)])
    check(ctx, k8, sizes, idx_bits, bits, False, width, what=what)
    b4 = min(bits, 26)
    bases = np.cumsum([0] + [1 << b4] * (len(sizes) - 1)).astype(np.int64)
    if bases[-1] + (1 << b4) <= 1 << 32:
        k4 = np.concatenate([rng.integers(0, 1 << b4, m, dtype=np.uint64) + U64(bases[s]) for s, m in enumerate(sizes)] + [np.zeros(0, U64)]).astype(U32)
        check(ctx, k4, sizes, 0, b4, True, width, bases=bases, what=what)


@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 2 * T + 1])
def test_one_segment_at_the_tile_edges(ctx, n):
    rng = np.random.default_rng(100 + n)
    for width in (8, 9):
        both_kinds(ctx, rng, [n], 34, width, "one segment")
        both_kinds(ctx, rng, [n], 17, width, "one segment")


@pytest.mark.parametrize("sizes", [[T, T - 1, T + 1, 2 * T, 1, 2 * T + 1], [0, T + 5, 0, 0, 300, 2 * T + 1, 0], [0, 0, 7], [5, 0], [1, 1, 1, T + 1]],
                         ids=["tile_edges", "empty_first_middle_last", "only_last", "only_first", "one_point_clouds"])
def test_segment_boundaries_and_empty_segments(ctx, sizes):
    rng = np.random.default_rng(len(sizes) * 1000 + sum(sizes))
    for width in (8, 9):
        both_kinds(ctx, rng, sizes, 34, width, "boundaries")
    both_kinds(ctx, rng, sizes, 9, 9, "boundaries, one place")


@pytest.mark.parametrize("nseg", [33, 64])
def test_more_segments_than_five_id_bits(ctx, nseg):
    rng = np.random.default_rng(nseg)
    sizes = [int(x) for x in rng.integers(100, 700, nseg)]
    both_kinds(ctx, rng, sizes, 34, 9, "every segment inside a tile")
    sizes[nseg // 2] = T + 7
    sizes[-1] = 0
    for width in (8, 9):
        both_kinds(ctx, rng, sizes, 34, width, "one segment beyond a tile")


def test_a_segment_beyond_one_chunk_of_tiles(ctx):
    """more than 64 tiles in a segment: the per-digit counts are scanned chunk by chunk (k_rss_chunks) and the chunks' totals per segment"""
    rng = np.random.default_rng(7)
    sizes = [65 * T + 1, 0, T + 1, 130 * T - 3]
    both_kinds(ctx, rng, sizes, 34, 9, "chunks")
    both_kinds(ctx, rng, sizes, 16, 8, "chunks")


def test_equal_keys_keep_their_order(ctx):
    for sizes in ([3 * T + 11], [700, 0, T + 1, 2 * T]):
        n = sum(sizes)
        for width in (8, 9):
            check(ctx, np.full(n, 0x2A5A5A5A5, U64) << U64(13), sizes, 13, 34, True, width, what="all equal")
            check(ctx, np.full(n, 0x00C3A5C3, U32), sizes, 0, 25, True, width, what="all equal")


def test_top_bit_of_the_top_place(ctx):
    """keys 0 and 2^(bits - 1) alone: the top place sees its two extreme digits and nothing else"""
    rng = np.random.default_rng(8)
    sizes = [T + 3, 2 * T - 1, 50]
    n = sum(sizes)
    for bits in (34, 27, 24, 9, 8):
        for width in (8, 9):
            k = (rng.integers(0, 2, n, dtype=np.uint64) << U64(bits - 1)) << U64(5)
            check(ctx, k, sizes, 5, bits, True, width, what="top bit")
            if bits <= 32:
                check(ctx, (k >> U64(5)).astype(U32), sizes, 0, bits, True, width, what="top bit")


@pytest.mark.parametrize("bits", [0, 1, 8, 9, 10, 16, 17, 18, 19, 24, 25, 27, 28, 32, 33, 34, 36, 37])
def test_bit_counts_around_the_multiples_of_the_digit_width(ctx, bits):
    rng = np.random.default_rng(200 + bits)
    sizes = [T + 1, 333, 2 * T]
    n = sum(sizes)
    for width in (8, 9):
        k = rng.integers(0, 1 << 63, n, dtype=np.uint64)  # noise above and below the sorted bits
        check(ctx, k, sizes, 11, bits, False, width, what="bit count")
        if bits <= 32:
            check(ctx, (k >> U64(20)).astype(U32), sizes, 0, bits, True, width, what="bit count")


def test_segments_of_different_bit_counts(ctx):
    """the plan is made for the widest segment: one of 5 key bits beside one of 20 and one of 34"""
    rng = np.random.default_rng(9)
    sizes = [T + 9, 2 * T + 1, 900]
    k = np.concatenate([rng.integers(0, 1 << b, m, dtype=np.uint64) for b, m in zip((5, 34, 20), sizes)])
    for width in (8, 9):
        check(ctx, k << U64(3), sizes, 3, 34, True, width, what="mixed bit counts")
    bases = [0, 32, 32 + (1 << 20)]
    k4 = np.concatenate([rng.integers(0, 1 << b, m, dtype=np.uint64) + U64(base) for b, m, base in zip((5, 20, 11), sizes, bases)]).astype(U32)
    for width in (8, 9):
        check(ctx, k4, sizes, 0, 20, True, width, bases=bases, what="mixed bit counts above a base")


def test_bad_arguments_are_refused(ctx):
    t = ctx.torch
    x = t.zeros(64, dtype=t.int32, device=ctx.dev)
    p, q = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(x.data_ptr() + 128)
    f = ctx.lib.ghicp_sort_segments
    ok = (ctypes.c_int64 * 3)(0, 8, 16)
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(2), ok, None, 0, 8, 0) == 0
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(2), (ctypes.c_int64 * 3)(1, 8, 16), None, 0, 8, 0) == 1  # not from 0
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(2), (ctypes.c_int64 * 3)(0, 9, 8), None, 0, 8, 0) == 1  # descending
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(0), ok, None, 0, 8, 0) == 1
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(65), ok, None, 0, 8, 0) == 1
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(2), ok, None, 30, 8, 0) == 1  # bits past the key
    assert f(ctx.h, 4, p, q, None, None, ctypes.c_int32(2), ok, None, 0, 8, 7) == 1  # digit width
    assert f(ctx.h, 4, p, p, None, None, ctypes.c_int32(2), ok, None, 0, 8, 0) == 1  # in place
    assert f(ctx.h, 8, p, q, None, None, ctypes.c_int32(2), ok, p, 0, 8, 0) == 1  # a base under 8-byte keys


def _same(a, b):
    ia, ib = a.info(), b.info()
    assert (ia.n, ia.m, ia.k, ia.variants, ia.feature) == (ib.n, ib.m, ib.k, ib.variants, ib.feature)
    assert ia.bbx_magnitude == ib.bbx_magnitude
    da, db = a.download(), b.download()
    for key in ("ds", "kp", "kp_xyz", "feat"):
        if da[key] is None or db[key] is None:
            assert da[key] is None and db[key] is None, key
        else:
            np.testing.assert_array_equal(da[key].cpu().numpy(), db[key].cpu().numpy(), err_msg=key)


@pytest.mark.parametrize("sizes", [[3000, T + 4], [3000, T + 1, T, 1, 5000]], ids=["two_clouds", "five_clouds"])
def test_batched_front_end_on_small_clouds_equals_cloud_by_cloud(ctx, api, synth, sizes):
    """raw clouds below a tile, exactly a tile and just above one: the handles of ghicp_clouds_recompute, whose voxel and grid sorts are
    segmented by cloud, are those of ghicp_cloud_recompute cloud by cloud, bit for bit"""
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_NN, dof=6, voxel=0.2, pattern=synth.bsc_pattern_glibc(), max_iter=40)
    src = synth.tls_pair(12_000, pair_id=31)
    raws = [(src.source if i % 2 == 0 else src.target)[i * 100:i * 100 + n] for i, n in enumerate(sizes)]
    single = [ctx.cloud_create(cfg, r) for r in raws]
    batch = [ctx.cloud_create(cfg, raws[0][:200]) for _ in raws]
    ctx.clouds_recompute(batch, raws)
    for c, d in zip(single, batch):
        _same(c, d)
    assert max(c.info().m for c in batch) > 500  # the comparison is not vacuous


def test_key_kernels_leave_the_first_place_histogram(ctx, api, synth):
    """The kernels that make the voxel keys and the cell keys leave the per-tile counts of the sort's first digit place, and the sort skips its
    own first histogram pass.  With the library's check on, every such sort takes the counts again from the keys it was given and compares the two
    tables word for word: one voxel sort and two grid sorts per batch here (raw and down-sampled clouds beyond a tile), none may differ -- and
    the handles are still those of the cloud-by-cloud front end."""
    cfg = api.pair_config(api.FEATURE_BSC, api.CORR_NN, dof=6, voxel=0.05, pattern=synth.bsc_pattern_glibc(), max_iter=40)
    src = synth.tls_pair(40_000, pair_id=33)
    raws = [src.source[:30_000], src.target[:T + 1], src.source[:0], src.target[5_000:5_000 + 2 * T + 9]]
    single = [ctx.cloud_create(cfg, r) for r in raws]
    batch = [ctx.cloud_create(cfg, raws[1][:100]) for _ in raws]

    def counters():
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert ctx.lib.ghicp_ctx_sort_hist_checks(ctx.h, ctypes.byref(a), ctypes.byref(b)) == 0
        return a.value, b.value

    c0, m0 = counters()
    assert ctx.lib.ghicp_ctx_set_sort_hist_check(ctx.h, 1) == 0
    try:
        ctx.clouds_recompute(batch, raws)
    finally:
        assert ctx.lib.ghicp_ctx_set_sort_hist_check(ctx.h, 0) == 0
    c1, m1 = counters()
    assert max(c.info().m for c in batch) > T, "the grids' sorts must be tiled for their key kernel to be covered"
    assert (c1 - c0, m1 - m0) == (3, 0)
    for c, d in zip(single, batch):
        _same(c, d)
    ctx.clouds_recompute(batch, raws)  # the check off again: nothing is counted
    assert counters() == (c1, m1)

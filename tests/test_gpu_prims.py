"""The device-wide primitives of prims.hip -- inclusive scan, select-by-flag, unique over a sorted run, stable radix sort -- on their own,
through the C ABI (ghicp_scan_inclusive_u32, ghicp_select_flagged, ghicp_unique_sorted_u32, ghicp_sort_pairs), against numpy in 64-bit.
Integer work with an exact answer: every comparison is assert_array_equal, nothing has a tolerance.

Every output and every in-place range is a window of a larger device tensor filled with a guard word; after each call every word outside
what the call may write (for select / unique: outside out[0 .. count)) must still be the guard.  An out-of-range store does not fault on the
GPU; this is how it is seen.

Sizes (SIZES): around the 16 items of a thread, the 64 of a wave, the 256 of a workgroup, the 4096 of a tile, 256 tiles exactly (one round of
k_scan_totals), 257 tiles (its second round, with a carry), and a ragged 3 000 017.

On the host SIMT interpreter (GHICP_SIM=1) every size of SIZES runs, every pattern, every offset (about a minute for the file).  Only the
8 388 608 / 8 388 609 cases of the sort -- the switch from the inline chunk sums to k_rs_bases -- are skipped there, like the 9 M cases of
test_sort_pairs_is_a_stable_sort_on_the_bit_range: a minute each on the interpreter; k_rs_bases itself has no size-dependent path beyond
its loop over the chunks."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIM = os.environ.get("GHICP_SIM") == "1"
TILE = 4096
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 4095, 4096, 4097, 8192, 65_537, 1_048_576, 1_048_577, 3_000_017]
GUARD_WORDS = 64
GUARD = np.int32(-1515870811)  # 0xA5A5A5A5
U32 = np.uint32


def framed(ctx, n, off=0):
    """(buf, window, lead): an int32 device tensor full of guard words and its window buf[lead : lead + n], which starts `off` words past
    a 256-byte boundary"""
    t = ctx.torch
    buf = t.full((3 * GUARD_WORDS + off + n,), int(GUARD), dtype=t.int32, device=ctx.dev)
    assert buf.data_ptr() % 4 == 0
    lead = GUARD_WORDS + (-(buf.data_ptr() // 4 + GUARD_WORDS)) % 64 + off
    win = buf[lead:lead + n]
    assert n == 0 or win.data_ptr() % 256 == 4 * off
    return buf, win, lead


def guards_intact(buf, lead, written):
    b = buf.cpu().numpy()
    assert lead >= GUARD_WORDS and b.shape[0] - (lead + written) >= GUARD_WORDS
    return bool((b[:lead] == GUARD).all() and (b[lead + written:] == GUARD).all())


def put(ctx, win, x):
    """x (uint32 array) into the window, in place"""
    if x.shape[0]:
        win.copy_(ctx.torch.from_numpy(x.view(np.int32)))


def as_u32(t):
    return t.cpu().numpy().view(U32)


# ------------------------------------------------------------------------------------------------------------------------ scan
def scan_ref(x):
    return (np.cumsum(x.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(U32)


def scan_inputs(rng, n):
    yield "full range (the sum wraps)", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    yield "all 0", np.zeros(n, U32)
    yield "all 1", np.ones(n, U32)
    yield "small", rng.integers(0, 8, n, dtype=np.uint64).astype(U32)
    if n:
        last_tile = (n - 1) // TILE * TILE
        mid_tile = (n - 1) // TILE // 2 * TILE
        for pos in sorted({0, mid_tile, mid_tile + TILE - 1, last_tile, last_tile - 1, n - 1}):  # first / last item of a tile, and the very last
            if 0 <= pos < n:
                x = np.zeros(n, U32)
                x[pos] = 0xDEADBEEF
                yield "single item at %d" % pos, x


def test_scan_at_every_size_base_offset_and_value_pattern(ctx):
    """ghicp_scan_inclusive_u32 in place on a window that starts 0, 1, 2 or 3 words past a 256-byte boundary (k_scan_apply's 16-byte path
    may be taken for the first of these only; batch_nms.hip scans `table + 1`).  Every size >= 17 has threads whose 16 items lie inside n and,
    unless n is a multiple of 16, one thread that straddles n."""
    rng = np.random.default_rng(11)
    for n in SIZES:
        for off in (0, 1, 2, 3):
            for what, x in scan_inputs(rng, n):
                buf, win, lead = framed(ctx, n, off)
                put(ctx, win, x)
                assert ctx.scan_inclusive(win).data_ptr() == win.data_ptr()
                np.testing.assert_array_equal(as_u32(win), scan_ref(x), err_msg="n=%d offset=%d %s" % (n, off, what))
                assert guards_intact(buf, lead, n), (n, off, what)


def test_scan_in_host_pointer_mode(ctx):
    """the same answers when the context stages host arrays (ghicp_ctx_set_host_pointers): in place in the caller's numpy array, guard words
    on both sides of the range, a base 0..3 words into the array"""
    lib = ctx.lib
    h = ctypes.c_void_p()
    assert lib.ghicp_ctx_create(0, ctypes.byref(h)) == 0
    try:
        assert lib.ghicp_ctx_set_host_pointers(h, 1) == 0
        rng = np.random.default_rng(12)
        for n in (0, 1, 17, 4097, 70_001, 1_048_577):
            for off in (0, 3):
                x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
                buf = np.full(GUARD_WORDS + off + n + GUARD_WORDS, GUARD.view(U32), U32)
                lead = GUARD_WORDS + off
                buf[lead:lead + n] = x
                p = ctypes.c_void_p(buf.ctypes.data + 4 * lead)
                assert lib.ghicp_scan_inclusive_u32(h, p, ctypes.c_int64(n)) == 0, lib.ghicp_last_error(h)
                np.testing.assert_array_equal(buf[lead:lead + n], scan_ref(x), err_msg="n=%d offset=%d" % (n, off))
                assert (buf[:lead] == GUARD.view(U32)).all() and (buf[lead + n:] == GUARD.view(U32)).all()
    finally:
        lib.ghicp_ctx_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------ select
def flag_patterns(rng, n):
    i = np.arange(n)
    yield "tile edges", ((i % TILE == 0) | (i % TILE == TILE - 1)).astype(np.uint8)
    yield "wave edges", ((i % 64 == 0) | (i % 64 == 63)).astype(np.uint8)
    yield "density 0.5", (rng.random(n) < 0.5).astype(np.uint8)
    yield "none", np.zeros(n, np.uint8)
    yield "all", np.ones(n, np.uint8)
    for pos in (0, n - 1):
        if n:
            f = np.zeros(n, np.uint8)
            f[pos] = 1
            yield "only item %d" % pos, f
    yield "density 0.001", (rng.random(n) < 0.001).astype(np.uint8)
    yield "density 0.999", (rng.random(n) < 0.999).astype(np.uint8)


def check_select(ctx, flags, vals, what):
    n = flags.shape[0]
    idx = np.flatnonzero(flags)
    want = idx.astype(U32) if vals is None else vals[idx]
    buf, win, lead = framed(ctx, n)
    got = ctx.select_flagged(flags, None if vals is None else vals.view(np.int32), out=win)
    assert got.shape[0] == idx.shape[0], (what, got.shape[0], idx.shape[0])  # *count
    assert got.shape[0] == 0 or got.data_ptr() == win.data_ptr()
    g = as_u32(got)
    np.testing.assert_array_equal(g, want, err_msg=what)
    if vals is None:
        assert (np.diff(g.astype(np.int64)) > 0).all(), what  # ascending positions
    assert guards_intact(buf, lead, idx.shape[0]), what  # nothing before out, nothing from out[count] on
    return g


def test_select_at_every_size_and_flag_pattern(ctx):
    """ghicp_select_flagged, positions (vals == NULL) and values: no hit, every item, item 0 or n - 1 alone, hits exactly on the first and
    last item of every tile / every wave, three densities; count, out[0 .. count) and the words from out[count] on"""
    rng = np.random.default_rng(13)
    for n in SIZES:
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        for what, f in flag_patterns(rng, n):
            check_select(ctx, f, None, "positions n=%d %s" % (n, what))
            check_select(ctx, f, vals, "values n=%d %s" % (n, what))


def test_select_counts_every_non_zero_flag_byte(ctx):
    """a flag is any non-zero byte: 0x02, 0x80 and 0xFF count like 0x01"""
    rng = np.random.default_rng(14)
    for n in (5, 64, 4097, 70_001):
        for byte in (0x02, 0x80, 0xFF):
            f = np.where(rng.random(n) < 0.3, byte, 0).astype(np.uint8)
            f[-1] = byte
            check_select(ctx, f, None, "n=%d byte %#x" % (n, byte))
        f = rng.choice(np.array([0, 0, 0, 1, 0x02, 0x80, 0xFF], np.uint8), n)
        check_select(ctx, f, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32), "n=%d mixed bytes" % n)


# ------------------------------------------------------------------------------------------------------------------------ unique
def keys_of_runs(heads):
    """ascending u32 keys with a new value wherever heads is set (heads[0] is): 0 first, 0xFFFFFFFF last"""
    ids = np.cumsum(heads) - 1
    table = np.arange(int(ids[-1]) + 1, dtype=np.uint64) * np.uint64(3)
    if table.shape[0] > 1:
        table[-1] = 0xFFFFFFFF
    return table[ids].astype(U32)


def key_patterns(rng, n):
    i = np.arange(n)
    for L in (4096, 4097):  # a run per tile: every head is the first item of a tile and key[i - 1] belongs to the tile before; then one item longer
        yield "runs of %d" % L, keys_of_runs(i % L == 0)
    yield "random runs, p = 0.3", keys_of_runs(np.r_[True, rng.random(n - 1) < 0.3])
    yield "all equal", np.full(n, 0x12345678, U32)
    yield "all equal to 0xFFFFFFFF", np.full(n, 0xFFFFFFFF, U32)
    yield "all distinct", keys_of_runs(np.ones(n, bool))
    yield "runs of 64", keys_of_runs(i % 64 == 0)
    h = rng.random(n) < 0.01
    h[::TILE] = True
    yield "random runs that also start with every tile", keys_of_runs(h)
    yield "random runs, p = 0.002", keys_of_runs(np.r_[True, rng.random(n - 1) < 0.002])


def check_unique(ctx, keys, what):
    n = keys.shape[0]
    want = keys[np.r_[True, keys[1:] != keys[:-1]]] if n else keys
    np.testing.assert_array_equal(want, np.unique(keys))  # (the input is ascending)
    buf, win, lead = framed(ctx, n)
    got = ctx.unique_sorted(keys.view(np.int32), out=win)
    assert got.shape[0] == want.shape[0], (what, got.shape[0], want.shape[0])
    np.testing.assert_array_equal(as_u32(got), want, err_msg=what)
    assert guards_intact(buf, lead, want.shape[0]), what
    return as_u32(got)


def test_unique_at_every_size_and_run_pattern(ctx):
    """ghicp_unique_sorted_u32: one run, n runs, runs that end exactly on a wave (64) or tile (4096) boundary and one item past it, runs
    that start with a tile, the keys 0 and 0xFFFFFFFF, random run lengths; count, out[0 .. count) and the words from out[count] on"""
    rng = np.random.default_rng(15)
    for n in SIZES:
        if n == 0:
            check_unique(ctx, np.zeros(0, U32), "n=0")
            continue
        for what, k in key_patterns(rng, n):
            check_unique(ctx, k, "n=%d %s" % (n, what))


# ------------------------------------------------------------------------------------------------------------------------ sort
def sort_ref(k, b, e):
    sub = (k.astype(np.uint64) >> np.uint64(b)) & np.uint64((1 << (e - b)) - 1)
    return np.argsort(sub, kind="stable")


def random_keys(rng, n, kb):
    if kb == 4:
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
    return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)


def check_sort(ctx, k, v, b, e, what):
    """keys (+ values) into guarded windows; against numpy's stable sort of the masked keys, inputs untouched"""
    n = k.shape[0]
    kb = k.dtype.itemsize
    t = ctx.torch
    order = sort_ref(k, b, e)
    ks = k.view(np.int32 if kb == 4 else np.int64)
    kd = t.from_numpy(ks.copy()).to(ctx.dev)
    kbuf, kwin, klead = framed(ctx, n * (kb // 4))
    ko = kwin.view(t.int64) if kb == 8 else kwin
    if v is None:
        out = ctx.sort_pairs(kd, None, b, e, keys_out=ko)
        assert out.data_ptr() == kwin.data_ptr()
    else:
        vd = t.from_numpy(v.copy()).to(ctx.dev)
        vbuf, vwin, vlead = framed(ctx, n)
        ctx.sort_pairs(kd, vd, b, e, keys_out=ko, vals_out=vwin)
        np.testing.assert_array_equal(vwin.cpu().numpy(), v[order], err_msg=what + " (values)")
        np.testing.assert_array_equal(vd.cpu().numpy(), v, err_msg=what + " (values in)")
        assert guards_intact(vbuf, vlead, n), what
    np.testing.assert_array_equal(ko.cpu().numpy(), ks[order], err_msg=what + " (keys)")
    np.testing.assert_array_equal(kd.cpu().numpy(), ks, err_msg=what + " (keys in)")
    assert guards_intact(kbuf, klead, n * (kb // 4)), what


def test_sort_on_both_sides_of_every_launch_sequence_switch(ctx):
    """The sort picks its launches by size: one workgroup (n <= 4096), one chunk of <= 64 tiles (k_rs_chunk_bases), <= 32 chunks (the scatter
    sums the chunk rows itself), k_rs_bases beyond.  The last and the first size of each, 4- and 8-byte keys, with and without values, two
    digit places (so that the spare buffer is in play)."""
    rng = np.random.default_rng(16)
    for n in [4096, 4097, 262_144, 262_145] + ([] if SIM else [8_388_608, 8_388_609]):
        for kb, b, e in ((4, 0, 16), (8, 27, 43)):
            k = random_keys(rng, n, kb)
            check_sort(ctx, k, rng.permutation(n).astype(np.int32), b, e, "n=%d %d-byte keys" % (n, kb))
            check_sort(ctx, k, None, b, e, "n=%d %d-byte keys, keys only" % (n, kb))


def test_sort_of_ordered_equal_and_single_digit_inputs(ctx):
    """already sorted, reverse sorted, all keys equal (the values must come out as they went in: stability on its own), and keys that all
    share the digit of one place (that pass sees one run per tile)"""
    rng = np.random.default_rng(17)
    for n in (1000, 4097, 70_001, 262_145, 1_000_003):
        iota = np.arange(n, dtype=np.int32)
        for kb in (4, 8):
            dt = U32 if kb == 4 else np.uint64
            bits = 24 if kb == 4 else 40
            asc = np.sort(random_keys(rng, n, kb) >> dt(8 * kb - bits))
            check_sort(ctx, asc, iota, 0, bits, "n=%d kb=%d sorted" % (n, kb))
            check_sort(ctx, asc[::-1].copy(), iota, 0, bits, "n=%d kb=%d reversed" % (n, kb))
            same = np.full(n, 0xC3A5C3A5, dt)
            check_sort(ctx, same, iota, 0, 8 * kb, "n=%d kb=%d all equal" % (n, kb))
            ko, vo = ctx.sort_pairs(same.view(np.int32 if kb == 4 else np.int64), iota, 0, 8 * kb)
            np.testing.assert_array_equal(vo.cpu().numpy(), iota)
            one = (random_keys(rng, n, kb) & ~dt(0xFF00)) | dt(0x5A00)  # digit place 1 is 0x5A everywhere
            check_sort(ctx, one, rng.permutation(n).astype(np.int32), 0, 24, "n=%d kb=%d one digit in place 1" % (n, kb))
            check_sort(ctx, one, None, 8, 16, "n=%d kb=%d that place alone" % (n, kb))


def test_sort_rejects_buffers_that_alias(ctx, api):
    """vals_in == vals_out, keys_out overlapping keys_in by a part of the range, an output on top of the OTHER input or the other output:
    GHICP_ERR_ARG, and not a word of the inputs changed (a single-pass sort would scatter into what other workgroups still read)"""
    rng = np.random.default_rng(18)
    t = ctx.torch
    for n in (100, 5000, 70_001):
        pool0 = rng.integers(-(1 << 31), 1 << 31, 6 * n, dtype=np.int64).astype(np.int32)
        pool = t.from_numpy(pool0.copy()).to(ctx.dev)
        k, v, ko, vo = pool[0:n], pool[2 * n:3 * n], pool[4 * n:5 * n], pool[5 * n:6 * n]
        bad = {
            "vals_in == vals_out": dict(keys=k, vals=v, keys_out=ko, vals_out=v),
            "keys_out overlaps the tail of keys_in": dict(keys=k, vals=v, keys_out=pool[n // 2:n // 2 + n], vals_out=vo),
            "keys_out overlaps the head of keys_in": dict(keys=pool[n // 2:n // 2 + n], vals=v, keys_out=k, vals_out=vo),
            "keys_out overlaps keys_in by one item": dict(keys=k, vals=None, keys_out=pool[n - 1:2 * n - 1], vals_out=None),
            "keys_out == vals_in": dict(keys=k, vals=v, keys_out=v, vals_out=vo),
            "vals_out == keys_in": dict(keys=k, vals=v, keys_out=ko, vals_out=k),
            "vals_out overlaps keys_out": dict(keys=k, vals=v, keys_out=ko, vals_out=pool[4 * n + n // 2:5 * n + n // 2]),
            "keys_out == keys_in": dict(keys=k, vals=None, keys_out=k, vals_out=None),
        }
        for what, a in bad.items():
            for bits in (8, 32):  # one pass straight into the output; four passes through the spare buffer
                with pytest.raises(api.GhicpError):
                    ctx.sort_pairs(a["keys"], a["vals"], 0, bits, keys_out=a["keys_out"], vals_out=a["vals_out"])
                np.testing.assert_array_equal(pool.cpu().numpy(), pool0, err_msg="n=%d %s" % (n, what))
        # 8-byte keys: the key range is 2 n words
        k8 = pool[0:2 * n].view(t.int64)
        with pytest.raises(api.GhicpError):
            ctx.sort_pairs(k8, v, 0, 64, keys_out=pool[n:3 * n].view(t.int64) if n % 2 == 0 else pool[n + 1:3 * n + 1].view(t.int64), vals_out=vo)
        np.testing.assert_array_equal(pool.cpu().numpy(), pool0)
        # buffers that merely touch are fine
        ctx.sort_pairs(k, v, 0, 32, keys_out=pool[n:2 * n], vals_out=pool[3 * n:4 * n])
        order = sort_ref(pool0[0:n].view(U32), 0, 32)
        np.testing.assert_array_equal(pool[n:2 * n].cpu().numpy(), pool0[0:n][order])
        np.testing.assert_array_equal(pool[3 * n:4 * n].cpu().numpy(), pool0[2 * n:3 * n][order])


def test_prims_reject_bad_arguments(ctx, api):
    t = ctx.torch
    lib, h = ctx.lib, ctx.h
    x = t.zeros(8, dtype=t.int32, device=ctx.dev)
    m = ctypes.c_int64(-1)
    p = ctypes.c_void_p(x.data_ptr())
    assert lib.ghicp_scan_inclusive_u32(h, p, ctypes.c_int64(-1)) == 1 and lib.ghicp_scan_inclusive_u32(h, None, ctypes.c_int64(4)) == 1
    assert lib.ghicp_scan_inclusive_u32(h, None, ctypes.c_int64(0)) == 0
    assert lib.ghicp_select_flagged(h, p, None, ctypes.c_int64(4), p, None) == 1  # no count
    assert lib.ghicp_select_flagged(h, p, None, ctypes.c_int64(4), p, ctypes.byref(m)) == 1  # out on top of flags
    assert lib.ghicp_select_flagged(h, None, None, ctypes.c_int64(0), None, ctypes.byref(m)) == 0 and m.value == 0
    m = ctypes.c_int64(-1)
    assert lib.ghicp_unique_sorted_u32(h, p, ctypes.c_int64(4), p, ctypes.byref(m)) == 1  # out on top of keys
    assert lib.ghicp_unique_sorted_u32(h, None, ctypes.c_int64(0), None, ctypes.byref(m)) == 0 and m.value == 0
    assert lib.ghicp_unique_sorted_u32(h, p, ctypes.c_int64(1 << 31), p, ctypes.byref(m)) == 1
    np.testing.assert_array_equal(x.cpu().numpy(), np.zeros(8, np.int32))


# ------------------------------------------------------------------------------------------------------------------------ determinism
def test_every_primitive_twice_on_the_same_input_is_bit_identical(ctx):
    rng = np.random.default_rng(19)
    t = ctx.torch
    for n in (4097, 1_048_577, 3_000_017):
        x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32)
        runs = []
        for _ in range(2):
            buf, win, lead = framed(ctx, n, 1)
            put(ctx, win, x)
            scan = as_u32(ctx.scan_inclusive(win)).copy()
            f = (x & U32(3) == 0).astype(np.uint8)
            sel = check_select(ctx, f, x, "n=%d" % n)
            pos = check_select(ctx, f, None, "n=%d" % n)
            uni = check_unique(ctx, np.sort(x >> U32(12)), "n=%d" % n)
            ko, vo = ctx.sort_pairs(x.view(np.int32), np.arange(n, dtype=np.int32), 4, 28)
            runs.append((scan, sel, pos, uni, ko.cpu().numpy(), vo.cpu().numpy()))
        for a, b in zip(*runs):
            assert a.tobytes() == b.tobytes()

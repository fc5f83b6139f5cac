"""Dynamic Huffman codes in the layers file's deflate blocks: crx_set_codes(CRX_CODES_DYNAMIC) of the companion library (include/cray_hip_exr.h,
c-ray_amd/csrc/exr_zip.h: k_zip_deflate_dynamic), Context.write_layers_exr(codes="dynamic") and the drop-in program's CRAY_HIP_EXR_CODES=dynamic.

The judge of a stream is Python's zlib (exr_reader.inflate_chunk); what is inside it — block types, the three code-length vectors of a dynamic block, token
counts — is read by the walker of tests/deflate_blocks.py, which inflates the stream itself and is anchored here against zlib on streams host zlib makes. The code
construction is tested through crx_debug_code_lengths against a package-merge reference (anchored here too). CPU tier: the two anchors, the adequacy of the size
condition's input, and this file's GPU tests run by a child pytest on the emulation."""
import contextlib
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import deflate_blocks as db
import test_exr_half as half_tests          # (its helpers: mixed_case, run_pack, one_row_shapes, layer_types; nothing of it is collected here)
import test_exr_zip as zip_tests            # (run_zip, crafted, size_sets)
from exr_reader import ALL_38, BYTES, F, H, inflate_chunk, raw_of, read_exr, run_dropin, split_chunks, typed_rows, zip_case, zip_forward, zip_inverse
from support import EMU_DIR, DeviceArray, ctx, dropin_env, dropin_paths, run_gpu_tests_on_emulation  # noqa: F401 (ctx: the fixture)

ALPHABETS = ((286, 15), (19, 7))          # (symbols, limit): the lit/len alphabet, the code-length alphabet
# Where the limit binds the device repairs the counts per length as zlib does instead of solving for the optimum: the worst ratio of its cost to package-merge's over
# the histograms of construction_histograms(), a deterministic integer function of them and the same on the device and on the emulation, measured on the emulation:
# 1.00054 (limit 15, the limit binds in 62 of the 215 histograms), 1.06412 (limit 7, in 66); asserted at the next half percent
WORST_EXCESS = {15: 1.005, 7: 1.065}


@pytest.fixture(scope="module")
def zctx(pkg, ctx):
    import cray_amd.exrzip as exrzip
    z = exrzip.ZipContext(0)
    yield z
    z.close()


@contextlib.contextmanager
def codes(zctx, name):
    """the calls inside run under crx_set_codes(name); fixed again behind them"""
    zctx.set_codes(name)
    try:
        yield
    finally:
        zctx.set_codes("fixed")


def seg():
    import cray_amd.exrzip as exrzip
    return exrzip.segment_bytes()


def check_blocks(data, n):
    """a deflated chunk under the walker: it inflates to what zlib inflates it to; one Huffman block a segment, fixed or dynamic, an empty stored block behind every
    one but the last, nothing else. Returns (segments coded with fixed codes, with dynamic codes, the blocks)."""
    out, blocks = db.walk_zlib(data)
    assert out == zlib.decompress(data) and len(out) == n
    coded = [b for b in blocks if b["btype"] != 0]
    assert len(coded) == -(-n // seg()) and len(blocks) == 2 * len(coded) - 1
    for k, b in enumerate(blocks):
        if k % 2:
            assert b["btype"] == 0 and b["stored"] == 0 and not b["final"], "between two segments: an empty stored block"
        else:
            assert b["btype"] in (1, 2) and b["final"] == (k == len(blocks) - 1)
    return sum(b["btype"] == 1 for b in coded), sum(b["btype"] == 2 for b in coded), blocks


def compare_modes(fixed, dynamic, want, row_bytes, h, lines):
    """(data, sizes) of the same call under both settings against the raw bytes `want`: every dynamic chunk inflates to its rows, is no larger than the fixed one, is
    raw only where the fixed one is (its stream is never longer), and holds only fixed and dynamic blocks and empty stored ones. Returns (segments coded fixed,
    coded dynamic)."""
    cf, cd = split_chunks(*fixed, row_bytes, 0, h, lines), split_chunks(*dynamic, row_bytes, 0, h, lines)
    assert raw_of(cf) == want and raw_of(cd) == want and len(want) == row_bytes * h
    tally = [0, 0]
    for k, ((_, df, n), (_, dd, _)) in enumerate(zip(cf, cd)):
        assert len(dd) <= len(df), (k, len(dd), len(df), "a chunk larger than in fixed mode")
        assert len(dd) < n or len(df) == n, (k, "raw under dynamic codes, deflated under fixed ones")
        if len(dd) < n:
            a, b, _ = check_blocks(dd, n)
            tally[0] += a
            tally[1] += b
    return tally


# ---- CPU tier: the support module's anchors -------------------------------------------------------------------------------------------------
def test_walker_is_anchored_against_zlib():
    """Streams host zlib makes — Z_FIXED, the default strategy, level 0, and a zlib stream with a full flush in it: the walker inflates each to what
    zlib.decompress gives, spans exactly the stream, and reports stored, fixed and dynamic blocks where they must occur; a dynamic block's vectors are complete
    codes of the stated sizes."""
    rng = np.random.default_rng(11)
    text = (b"the quick brown fox jumps over the lazy dog, " * 40) + bytes(rng.integers(100, 140, 3000, dtype=np.uint8)) + bytes(1000) + bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    seen = set()
    for level, strategy in ((1, zlib.Z_FIXED), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED)):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        stream = c.compress(text) + c.flush()
        out, blocks, used = db.walk(stream)
        assert out == zlib.decompress(stream, -15) == text and used == len(stream)
        kinds = {b["btype"] for b in blocks}
        assert kinds == ({0} if level == 0 else {1} if strategy == zlib.Z_FIXED else {2}), (level, strategy, kinds)
        seen |= kinds
        assert blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1]) and blocks[0]["span"][0] == 0 and blocks[-1]["span"][1] == len(stream)
        for b in blocks:
            if b["btype"] == 2:
                assert 257 <= len(b["lit"]) <= 286 and 1 <= len(b["dist"]) <= 30 and len(b["cl"]) == 19 and 4 <= b["hclen"] <= 19
                assert db.kraft(b["lit"]) == 1 and db.kraft(b["cl"]) == 1 and b["matches"] > 0 and b["literals"] > 0
    assert seen == {0, 1, 2}
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY)          # a zlib stream with an empty stored block (a full flush) between two dynamic ones
    stream = c.compress(text[:3000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[3000:]) + c.flush()
    out, blocks = db.walk_zlib(stream)
    assert out == text and [b["btype"] for b in blocks][:2] == [2, 0] and blocks[1]["stored"] == 0
    # the single-symbol codes inflate allows, and the incomplete ones it refuses
    assert db.canonical([0, 1, 0])[1] == [(1, 1), None]
    with pytest.raises(AssertionError):
        db.canonical([1, 1, 1])


def fibonacci_weights():
    """1, 1, 1, 2, 3, 5, ... 987: seventeen weights, 2 584 in all. Every merge but the first meets a tie: a Huffman tree of these is 16 deep if ties go to the
    nodes and 9 deep if they go to the leaves (the tree of least depth, which the device builds) — both of the same cost"""
    w = [1, 1, 1]
    while len(w) < 17:
        w.append(w[-1] + w[-2])
    return w


def deep_weights(depth):
    """1, 1, 1, 3, 4, 7, 11, 18, ...: every weight one more than all but the last before it together, so each merge joins the node made so far with the next
    leaf and no tie occurs: depth + 1 weights whose Huffman tree, whatever the tie rule, is `depth` deep — 3 570 in all for depth 16, 75 for depth 8"""
    w = [1, 1, 1]
    while len(w) < depth + 1:
        w.append(sum(w[:-1]) + 1)
    return w


def test_package_merge_is_anchored():
    """Kraft sum exactly 1 whether the limit binds or not; no length above the limit; Huffman's cost where Huffman's tree stays within the limit, more where it
    does not; the textbook case 1 1 1 2 3 5 ... whose tree is 16 deep."""
    rng = np.random.default_rng(5)
    fib, deep = fibonacci_weights(), deep_weights(16)
    assert sum(fib) == 2584 and max(db.huffman_lengths(fib)) == 9 and deep[:8] == [1, 1, 1, 3, 4, 7, 11, 18]
    assert sum(deep) == 3570 and max(db.huffman_lengths(deep)) == 16 and sum(deep[:9]) == 75 and max(db.huffman_lengths(deep[:9])) == 8
    assert db.huffman_lengths([5, 0, 0]) == [1, 0, 0] == db.package_merge([5, 0, 0], 7) and db.huffman_lengths([0, 0]) == [0, 0]
    assert sorted(db.huffman_lengths([1, 1, 2, 4])) == [1, 2, 3, 3] and db.package_merge([1, 1, 2, 4], 2) == [2, 2, 2, 2]
    cases = [fib, deep, deep[::-1], deep[:9], [1 << k for k in range(22)], [3] * 286, [7, 9]]
    for _ in range(60):
        n = int(rng.integers(2, 287))
        f = rng.integers(1, 1 + int(rng.choice([3, 40, 4000])), n) * (rng.random(n) < rng.choice([0.2, 0.7, 1.0]))
        if np.count_nonzero(f) >= 2:
            cases.append([int(v) for v in f])
    bound = 0
    for f in cases:
        plain = db.huffman_lengths(f)
        for limit in (7, 15):
            if np.count_nonzero(f) > 2 ** limit:
                continue
            got = db.package_merge(f, limit)
            assert db.kraft(got) == 1 and max(got) <= limit and all((b > 0) == (v > 0) for b, v in zip(got, f))
            if max(plain) <= limit:
                assert db.cost(f, got) == db.cost(f, plain)
            else:
                assert db.cost(f, got) > db.cost(f, plain)
                bound += 1
    assert bound >= 10, "the limit binds in enough of the cases"


# ---- CPU tier: the size condition's input --------------------------------------------------------------------------------------------------------
def size_planes():
    """six smooth, noisy colour-like planes, 160 x 96"""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:96, 0:160]
    return [np.abs((0.2 + 0.6 * (0.5 + 0.5 * np.sin(xx / 25 + k)) * (0.3 + yy / 96)) * (1 + 0.08 * rng.standard_normal((96, 160)))).astype(np.float32) for k in range(6)]


def yardstick(rows, lines):
    """host zlib level 1 per chunk of `lines` rows on the same T', 8-byte headers, raw where not shorter: (bytes with Z_FIXED, with the default strategy, raw bytes)"""
    fixed = dynamic = total = 0
    for y in range(0, rows.shape[0], lines):
        raw = rows[y:y + lines].tobytes()
        tp = zip_forward(raw)
        for strategy in (zlib.Z_FIXED, zlib.Z_DEFAULT_STRATEGY):
            c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, strategy)
            size = 8 + min(len(c.compress(tp) + c.flush()), len(raw))
            if strategy == zlib.Z_FIXED:
                fixed += size
            else:
                dynamic += size
        total += 8 + len(raw)
    return fixed, dynamic, total


def size_rows():
    planes = [p.view(np.uint32) for p in size_planes()]
    return planes, typed_rows(np.stack(planes, axis=1), [H] * 6)


def test_size_condition_input_is_adequate():
    """The yardstick alone, without a device: on the six HALF planes host zlib with dynamic codes allowed is at least 8 % below host zlib with fixed codes."""
    _, rows = size_rows()
    fixed, dynamic, total = yardstick(rows, 16)
    print(f"yardstick: fixed {fixed / total:.4f}, dynamic allowed {dynamic / total:.4f} of {total} bytes, gain {1 - dynamic / fixed:.4f}")
    assert rows.shape == (96, 6 * 2 * 160) and 1 - dynamic / fixed >= 0.08
    assert abs(fixed / total - 0.7508) < 0.002 and abs(dynamic / total - 0.6788) < 0.002


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lines", [1, 16])
def test_round_trip_in_dynamic_mode(lines, pkg, ctx, zctx):
    """The all-FLOAT cases of zip_case and the HALF / FLOAT shapes of tests/test_exr_half.py — a single HALF channel of width 1 (n = 2), n = 2 (mod 4), rows of
    S - 2 .. 2 S + 2 bytes, 161 x 75 with the layers file's 38 channels — under CRX_CODES_DYNAMIC: every chunk inflates to the rows the packer and numpy give, none
    is larger than under the fixed codes, and the walker finds fixed blocks, dynamic blocks and empty stored ones only; both codings occur."""
    kind = 2 if lines == 1 else 3
    total = [0, 0]
    for name in ("3x2x7", "40x17x5", "161x75x38"):
        case = zip_case(name)
        w, h, nch = case[0], case[1], len(case[3])
        fixed = zip_tests.run_zip(pkg, ctx, zctx, case, lines)
        with codes(zctx, "dynamic"):
            dynamic = zip_tests.run_zip(pkg, ctx, zctx, case, lines)
        assert fixed[2] == dynamic[2]
        t = compare_modes(fixed[:2], dynamic[:2], fixed[2], 4 * nch * w, h, lines)
        total = [total[0] + t[0], total[1] + t[1]]
    shapes = [(1, 1, [H]), (3, 2, [H, F, H, H]), (5, 17, [F, H]), (67, 5, [H, H, H]), (40, 17, [H, F, F, H, F]), (9, 75, [F, H]), (161, 75, half_tests.layer_types(pkg))]
    shapes += [(w, 1, types) for w, types in half_tests.one_row_shapes()]
    assert [w * sum(BYTES[t] for t in types) - seg() for w, h, types in shapes[-5:]] == [-2, 0, 2, seg() - 2, seg() + 2]
    for w, h, types in shapes:
        case = half_tests.mixed_case(w, h, types)
        row_bytes = w * sum(BYTES[t] for t in types)
        fixed = half_tests.run_pack(pkg, ctx, zctx, case, kind)
        with codes(zctx, "dynamic"):
            dynamic = half_tests.run_pack(pkg, ctx, zctx, case, kind)
        assert fixed[2] == dynamic[2]
        t = compare_modes(fixed[:2], dynamic[:2], fixed[2], row_bytes, h, lines)
        total = [total[0] + t[0], total[1] + t[1]]
        if (w, h) == (1, 1):
            assert dynamic[0] == struct.pack("<ii", 0, 2) + fixed[2], "2 bytes come back raw"
    print(f"lines {lines}: {total[0]} segments coded with the fixed codes, {total[1]} with dynamic ones")
    assert total[0] > 0 and total[1] > 0, "both codings occur"
    assert zctx.codes == "fixed"


def de_bruijn(k, n):
    """the lexicographically least de Bruijn sequence B(k, n): k^n symbols, every n-gram once around the cycle"""
    a, out = [0] * (k * n), []

    def step(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            step(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                step(t + 1, t)
    step(1, 1)
    return out


def pack_rows(pkg, ctx, zctx, tps, name):
    """one FLOAT channel, ZIPS: row k's chunk has T' = tps[k]; the chunks [(y, data, n)] under the codes `name`"""
    plane = zip_tests.crafted(tps)
    h, w = plane.shape
    dev = DeviceArray(pkg, plane.reshape(h, w, 1), np.uint32)
    ctx.synchronize()
    with codes(zctx, name):
        data, sizes = zctx.pack_zip([(dev.ptr, 1, 0)], w, h, 1)
    chunks = split_chunks(data, sizes, 4 * w, 0, h, 1)
    assert [inflate_chunk(d, n) for _, d, n in chunks] == [zip_inverse(t) for t in tps]
    return chunks


@pytest.mark.gpu
def test_crafted_transformed_bytes(pkg, ctx, zctx):
    """T' built on the host, one segment a chunk: one byte value throughout — a literal, then matches of distance 1 alone: a distance code of a single symbol of
    length 1 —; a de Bruijn sequence B(16, 3) around 128 — no trigram twice, so no match: HDIST = 1 with a zero length, at most 0.55 n where the fixed codes leave
    the chunk raw —; that segment followed by a segment of noise in one chunk; and the noise set of tests/test_exr_zip.py, raw under dynamic codes too."""
    S = seg()
    assert S == 4096
    rng = np.random.default_rng(21)
    sequence = bytes(120 + v for v in de_bruijn(16, 3))
    assert len(sequence) == S and len({sequence[i:i + 3] for i in range(S - 2)}) == S - 2 and set(sequence) == set(range(120, 136))
    constant = bytes([77]) * S
    for name in ("fixed", "dynamic"):
        (_, one, n), (_, bruijn, _) = pack_rows(pkg, ctx, zctx, [constant, sequence], name)
        assert n == S and len(one) < 64
        if name == "fixed":
            assert len(bruijn) == n, "8 bits a literal: raw under the fixed codes"
            continue
        _, coded, blocks = check_blocks(one, n)
        b = blocks[0]
        assert coded == 1 and b["literals"] == 1 and b["matches"] >= 16 and b["distances"] == {0} and b["dist"] == [1], "one distance symbol: a code of length 1"
        _, coded, blocks = check_blocks(bruijn, n)
        b = blocks[0]
        assert coded == 1 and b["matches"] == 0 and b["literals"] == S and b["dist"] == [0], "no match: HDIST = 1, a length of zero"
        assert sorted(v for v in b["lit"] if v) == [4] * 15 + [5, 5], "sixteen equally frequent literals and the end of block"
        print(f"de Bruijn segment: {len(bruijn)} of {n} bytes")
        assert len(bruijn) <= 0.55 * n
    noise = bytes(rng.integers(0, 256, S, dtype=np.uint8))
    (_, two, n), = pack_rows(pkg, ctx, zctx, [sequence + noise], "dynamic")
    assert n == 2 * S and len(two) < n
    _, _, blocks = check_blocks(two, n)
    assert blocks[0]["btype"] == 2 and blocks[0]["matches"] == 0 and blocks[0]["literals"] == S
    planes = [np.ascontiguousarray(p).view(np.uint32) for p in zip_tests.size_sets()["noise"]]
    words = np.ascontiguousarray(np.stack(planes, axis=2))
    dev = DeviceArray(pkg, words, np.uint32)
    ch = [(dev.ptr, 3, c) for c in range(3)]
    ctx.synchronize()
    for lines in (1, 16):
        with codes(zctx, "dynamic"):
            data, sizes = zctx.pack_zip(ch, 160, 96, lines)
        chunks = split_chunks(data, sizes, 4 * 3 * 160, 0, 96, lines)
        assert all(len(d) == n for _, d, n in chunks), "noise stays raw"
        assert raw_of(chunks) == np.stack(planes, axis=1).astype("<u4").tobytes()


def construction_histograms(symbols, limit):
    """[(what, counts)] over an alphabet of `symbols`: the edges of the construction, the weights that drive Huffman's tree past the limit, 200 random ones"""
    rng = np.random.default_rng(100 + limit)
    fib = deep_weights(limit + 1)          # (the weights 1 1 1 2 3 5 ... do not bind the limit under the tree of least depth: they are a case further down)
    assert sum(fib) <= 4097 and max(db.huffman_lengths(fib)) == limit + 1

    def spread(values, at):
        f = np.zeros(symbols, np.int64)
        f[np.asarray(at)] = values
        return f
    out = [("one symbol, the first", spread([9], [0])), ("one symbol, the last", spread([1], [symbols - 1])), ("one symbol, inside", spread([4097], [symbols // 2])),
           ("two symbols", spread([1, 1], [0, symbols - 1])), ("two unequal symbols", spread([4000, 1], [3, 4])), ("all equal", np.full(symbols, 3, np.int64)),
           ("all equal but one", spread([500], [7]) + 1),
           ("the deep tree", spread(fib, np.arange(len(fib)))), ("the deep tree reversed", spread(fib[::-1], np.arange(len(fib)))),
           ("the deep tree at the end", spread(fib, symbols - len(fib) + np.arange(len(fib)))),
           ("the deep tree shuffled", spread(fib, rng.permutation(symbols)[:len(fib)])), ("the deep tree among ones", np.maximum(spread(fib, rng.permutation(symbols)[:len(fib)]), 1)[:symbols]),
           ("1 1 1 2 3 5 ...", spread(fibonacci_weights()[:min(symbols, 17)], np.arange(min(symbols, 17)))),
           ("powers of two", spread([1 << k for k in range(min(symbols, 22))], np.arange(min(symbols, 22)))),
           ("powers of two shuffled", spread([1 << k for k in range(min(symbols, 22))], rng.permutation(symbols)[:min(symbols, 22)]))]
    for k in range(200):
        kind = k % 4
        if kind == 0:
            f = rng.integers(1, 60, symbols)
        elif kind == 1:
            f = np.floor(4000 * rng.random(symbols) ** 12).astype(np.int64) + 1          # a few heavy symbols, many rare ones
        elif kind == 2:
            f = (1 << rng.integers(0, 18 if symbols <= 19 else 13, symbols)).astype(np.int64)          # (the sum stays below 2^23)
        else:
            f = np.floor(rng.exponential(30.0, symbols)).astype(np.int64) + 1
        f = f * (rng.random(symbols) < rng.choice([0.15, 0.5, 0.9]))
        out.append((f"random {k}", f.astype(np.int64)))
    assert all(int(f.sum()) < 2 ** 23 for _, f in out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("symbols,limit", ALPHABETS)
def test_code_construction(symbols, limit, zctx):
    """crx_debug_code_lengths — the device function the deflate kernel calls — on construction_histograms(): a zero count gets length 0, a used symbol 1 .. limit;
    two or more used symbols make a complete code, Kraft sum exactly 1; one used symbol gets length 1 and nothing else a length; the cost equals Huffman's (and
    package-merge's) wherever Huffman's tree of least depth stays within the limit; where the limit binds the cost stays within WORST_EXCESS of package-merge's
    optimum."""
    cases = construction_histograms(symbols, limit)
    freq = np.stack([f for _, f in cases]).astype(np.uint32)
    lengths = zctx.code_lengths(freq, limit)
    assert lengths.shape == freq.shape and lengths.dtype == np.uint8
    assert np.array_equal(zctx.code_lengths(freq[3], limit), lengths[3]), "one histogram alone"
    worst, bound = 1.0, 0
    for (what, f), got in zip(cases, lengths.tolist()):
        f = [int(v) for v in f]
        used = sum(v > 0 for v in f)
        assert all((b == 0) == (v == 0) for b, v in zip(got, f)) and max(got, default=0) <= limit, what
        if used == 0:
            continue
        if used == 1:
            assert sorted(got)[-2:] == [0, 1], what
            continue
        assert db.kraft(got) == 1, (what, db.kraft(got))
        plain, best = db.huffman_lengths(f), db.package_merge(f, limit)
        if max(plain) <= limit:
            assert db.cost(f, got) == db.cost(f, plain) == db.cost(f, best), what
        else:
            ratio = db.cost(f, got) / db.cost(f, best)
            bound += 1
            worst = max(worst, ratio)
            assert 1.0 <= ratio <= WORST_EXCESS[limit], (what, ratio)
    print(f"limit {limit}: the limit binds in {bound} of {len(cases)} histograms, worst cost {worst:.5f} of package-merge's")
    assert bound >= 10
    L = zctx.L          # refusals
    out = np.zeros(symbols, np.uint8)
    ok = np.ones(symbols, np.uint32)
    big = np.full(symbols, 2 ** 23 // symbols + 1, np.uint32)
    for args in ((None, ok.ctypes.data, symbols, limit, 1, out.ctypes.data), (zctx.h, None, symbols, limit, 1, out.ctypes.data), (zctx.h, ok.ctypes.data, symbols, limit, 1, None),
                 (zctx.h, ok.ctypes.data, 0, limit, 1, out.ctypes.data), (zctx.h, ok.ctypes.data, 289, limit, 1, out.ctypes.data), (zctx.h, ok.ctypes.data, symbols, 8, 1, out.ctypes.data),
                 (zctx.h, ok.ctypes.data, symbols, 16, 1, out.ctypes.data), (zctx.h, big.ctypes.data, symbols, limit, 1, out.ctypes.data)):
        assert L.crx_debug_code_lengths(*args) == -1 and b"crx_debug_code_lengths" in L.crx_last_error(), args[2:5]
    assert not out.any()


@pytest.mark.gpu
def test_size_conditions_in_dynamic_mode(pkg, ctx, zctx):
    """ZIP, 160 x 96. Six HALF colour-like planes: the yardstick first (host zlib level 1 with dynamic codes allowed at least 8 % below Z_FIXED), then the device,
    whose dynamic size must lie below its own fixed size by at least half the yardstick's relative gain — a floor against a builder that falls back to fixed; both
    figures are printed. On the mixed FLOAT set of tests/test_exr_zip.py dynamic codes cost nothing: no chunk larger, 1 and 16 lines."""
    planes, rows = size_rows()
    yf, yd, total = yardstick(rows, 16)
    gain = 1 - yd / yf
    assert gain >= 0.08, gain
    words = np.ascontiguousarray(np.stack(planes, axis=2))
    dev = DeviceArray(pkg, words, np.uint32)
    ch = [(dev.ptr, 6, c) for c in range(6)]
    ctx.synchronize()
    fixed = zctx.pack(ch, 160, 96, 3, [H] * 6)
    with codes(zctx, "dynamic"):
        dynamic = zctx.pack(ch, 160, 96, 3, [H] * 6)
    t = compare_modes(fixed, dynamic, rows.tobytes(), rows.shape[1], 96, 16)
    mine = 1 - len(dynamic[0]) / len(fixed[0])
    print(f"six HALF planes, ZIP: yardstick {yf / total:.4f} -> {yd / total:.4f} of raw (gain {gain:.4f}); device {len(fixed[0]) / total:.4f} -> {len(dynamic[0]) / total:.4f} "
          f"(gain {mine:.4f}); {t[1]} of {t[0] + t[1]} segments dynamic")
    assert mine >= 0.5 * gain, (mine, gain)
    planes = [np.ascontiguousarray(p).view(np.uint32) for p in zip_tests.size_sets()["mixed"]]
    nch = len(planes)
    dev = DeviceArray(pkg, np.ascontiguousarray(np.stack(planes, axis=2)), np.uint32)
    ch = [(dev.ptr, nch, c) for c in range(nch)]
    raw = np.stack(planes, axis=1).astype("<u4").tobytes()
    ctx.synchronize()
    for lines in (1, 16):
        fixed = zctx.pack_zip(ch, 160, 96, lines)
        with codes(zctx, "dynamic"):
            dynamic = zctx.pack_zip(ch, 160, 96, lines)
        compare_modes(fixed, dynamic, raw, 4 * nch * 160, 96, lines)
        print(f"mixed, lines {lines}: fixed {len(fixed[0]) / len(raw):.4f}, dynamic {len(dynamic[0]) / len(raw):.4f} of raw")


@pytest.mark.gpu
def test_determinism_row_ranges_and_the_setting(pkg, ctx, zctx):
    """67 x 75, nine mixed channels, ZIPS and ZIP under dynamic codes: two calls give equal bytes; first_row ranges concatenate to the whole; back on fixed codes the
    bytes are a fresh context's; crx_get_codes reads back what was set; a refused value or a NULL context answers CRH_ERR_INVALID and changes nothing."""
    import cray_amd.exrzip as exrzip
    case = half_tests.mixed_case(67, 75, [H, F, H, H, F, F, H, F, H])
    h = case[1]
    L, invalid = zctx.L, pkg.abi.ERR_INVALID
    assert zctx.codes == "fixed"
    fresh = exrzip.ZipContext(0)
    assert fresh.codes == "fixed"
    for kind in (2, 3):
        want_fixed = half_tests.run_pack(pkg, ctx, fresh, case, kind)[0]
        with codes(zctx, "dynamic"):
            assert zctx.codes == "dynamic"
            whole, sizes, _ = half_tests.run_pack(pkg, ctx, zctx, case, kind)
            again, sizes2, _ = half_tests.run_pack(pkg, ctx, zctx, case, kind)
            assert whole == again and np.array_equal(sizes, sizes2) and int(sizes.sum()) == len(whole)
            ranges = ((0, 16), (16, 32), (48, h - 48))
            parts = [half_tests.run_pack(pkg, ctx, zctx, case, kind, first_row=f, row_count=r) for f, r in ranges]
            assert b"".join(p[0] for p in parts) == whole and np.array_equal(np.concatenate([p[1] for p in parts]), sizes)
            assert half_tests.run_pack(pkg, ctx, zctx, case, 0)[0] == half_tests.run_pack(pkg, ctx, fresh, case, 0)[0], "compression 0 ignores the setting"
        assert zctx.codes == "fixed"
        assert whole != want_fixed and len(whole) < len(want_fixed)
        assert half_tests.run_pack(pkg, ctx, zctx, case, kind)[0] == want_fixed, "dynamic, then fixed: a fresh context's bytes"
    fresh.close()
    value = C.c_int(-5)
    for setting in (1, 0, 1):
        assert L.crx_set_codes(zctx.h, setting) == 0 and L.crx_get_codes(zctx.h, C.byref(value)) == 0 and value.value == setting
        for bad in (2, -1, 255, 1 << 16):
            assert L.crx_set_codes(zctx.h, bad) == invalid and b"crx_set_codes" in L.crx_last_error()
            assert L.crx_get_codes(zctx.h, C.byref(value)) == 0 and value.value == setting, "a refused value leaves the setting"
    assert L.crx_set_codes(None, 1) == invalid and L.crx_set_codes(None, 0) == invalid
    value.value = -5
    assert L.crx_get_codes(None, C.byref(value)) == invalid and value.value == -5 and L.crx_get_codes(zctx.h, None) == invalid
    with pytest.raises(ValueError):
        zctx.set_codes("best")
    assert zctx.codes == "dynamic"
    zctx.set_codes("fixed")


@pytest.mark.gpu
def test_rendered_layers_file_with_dynamic_codes(pkg, ctx, golden_blob, manifest, tmp_path):
    """cfg1_scene with every layer, compression "zip", half=True: the codes="dynamic" file reads back, plane for plane and bit for bit, as the codes="fixed" file,
    and is no larger; the default is "fixed"; the companion context's setting is put back; with compression "none" the argument changes nothing; another value
    raises ValueError and writes nothing."""
    m = manifest["cfg1_scene"]
    w, h, n = m["width"], m["height"], 4
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    fb, dn, aov = ctx.framebuffer(w, h), ctx.framebuffer(w, h), ctx.aov_buffer(w, h)
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_region(fb, w, h, n, 4)
    ctx.render_aov(aov, w, h, n)
    ctx.render_ids(bi, bm, w, h, n)
    ctx.denoise(fb, aov, w, h, out=dn, iterations=2)
    kw = dict(aov=aov, denoised=dn, instance_ids=bi, material_ids=bm)
    names = sorted(ALL_38, key=lambda s: s.encode())
    files = {}
    for what, more in (("default", {}), ("fixed", dict(codes="fixed")), ("dynamic", dict(codes="dynamic")), ("dynamic in parts", dict(codes="dynamic", chunk_rows=40))):
        path = str(tmp_path / f"{what}.exr")
        assert ctx.write_layers_exr(path, w, h, fb, compression="zip", half=True, **more, **kw) == names
        files[what] = open(path, "rb").read()
        assert ctx._zip_context().codes == "fixed", "the setting is put back"
    assert files["default"] == files["fixed"] and files["dynamic"] == files["dynamic in parts"]
    f0, f1 = read_exr(files["fixed"]), read_exr(files["dynamic"])
    assert (f1["compression"], f1["names"], f1["types"], f1["attrs"]) == (3, names, f0["types"], f0["attrs"])
    for c in names:
        assert f1["planes"][c].dtype == f0["planes"][c].dtype and np.array_equal(f1["planes"][c], f0["planes"][c]), c
    assert all(b <= a for (_, a, _), (_, b, _) in zip(f0["chunks"], f1["chunks"])) and len(files["dynamic"]) < len(files["fixed"])
    print(f"zip, half: dynamic {len(files['dynamic'])} of {len(files['fixed'])} bytes = {len(files['dynamic']) / len(files['fixed']):.4f}")
    ctx._zip_context().set_codes("dynamic")          # a setting of the caller's survives a call that asks for the other
    ctx.write_layers_exr(str(tmp_path / "again.exr"), w, h, fb, compression="zip", half=True, codes="fixed", **kw)
    assert ctx._zip_context().codes == "dynamic" and open(str(tmp_path / "again.exr"), "rb").read() == files["fixed"]
    ctx._zip_context().set_codes("fixed")
    for half in (False, True):
        a, b = str(tmp_path / "none_a.exr"), str(tmp_path / "none_b.exr")
        ctx.write_layers_exr(a, w, h, fb, compression="none", half=half, **kw)
        ctx.write_layers_exr(b, w, h, fb, compression="none", half=half, codes="dynamic", **kw)
        assert open(a, "rb").read() == open(b, "rb").read()
    for bad in ("best", None, 1):
        with pytest.raises(ValueError):
            ctx.write_layers_exr(str(tmp_path / "bad.exr"), w, h, fb, compression="zip", codes=bad, **kw)
    assert not os.path.exists(str(tmp_path / "bad.exr"))


@pytest.mark.gpu
def test_dropin_program_writes_the_dynamic_layers_file(pkg, ctx, manifest, golden_blob, tmp_path):
    """c-ray-hip with CRAY_HIP_EXR=1 CRAY_HIP_EXR_COMPRESSION=zip CRAY_HIP_EXR_HALF=1 CRAY_HIP_EXR_CODES=dynamic: the layers file is, byte for byte, what
    Context.write_layers_exr(compression="zip", half=True, codes="dynamic") writes from the same buffers and names, and smaller than with a value that is not
    `dynamic`, which leaves the file as it is without the variable; every other file of the run is unchanged."""
    import json
    if not dropin_paths()[2]:
        pytest.skip("c-ray-hip or the asset overlay is not built (needs the reference's sources at build time)")
    m = manifest["cfg1_scene"]
    w, h, s = m["width"], m["height"], m["samples"]
    env = dict(dropin_env(), CRAY_HIP_IDS="4", CRAY_HIP_EXR="1", CRAY_HIP_EXR_COMPRESSION="zip", CRAY_HIP_EXR_HALF="1")
    plain, _ = run_dropin(manifest, str(tmp_path / "plain"), dict(env, CRAY_HIP_EXR_CODES="1"))
    files, _ = run_dropin(manifest, str(tmp_path / "dynamic"), dict(env, CRAY_HIP_EXR_CODES="dynamic"))
    assert sorted(files) == sorted(plain)
    for name, data in plain.items():
        assert name == "refrun_layers_0000.exr" or files[name] == data, f"{name} changed"
    data = files["refrun_layers_0000.exr"]
    f, f0 = read_exr(data), read_exr(plain["refrun_layers_0000.exr"])
    assert f["compression"] == 3 and len(data) < len(plain["refrun_layers_0000.exr"]) and f["types"] == f0["types"]
    for c in f0["names"]:
        assert np.array_equal(f["planes"][c], f0["planes"][c]), c
    inst = list(json.loads(f["attrs"]["cryptomatte/3ae39a5/manifest"][1].decode()))
    mat = list(json.loads(f["attrs"]["cryptomatte/be359d6/manifest"][1].decode()))
    frame = np.frombuffer(files["frame.f32"], np.uint32).reshape(h, w, 3)
    guides = np.frombuffer(files["aov.f32"], np.uint32).reshape(h, w, 8)
    denoised = np.frombuffer(files["denoised.f32"], np.uint32).reshape(h, w, 3)
    ctx.upload(pkg.api.Scene(golden_blob("cfg1_scene")))
    bi, bm = ctx.ids_buffer(w, h), ctx.ids_buffer(w, h)
    ctx.render_ids(bi, bm, w, h, s, pass_count=min(4, s))
    dev = [DeviceArray(pkg, a, np.uint32) for a in (frame, guides, denoised)]
    kw = dict(aov=dev[1].ptr, denoised=dev[2].ptr, instance_ids=bi, material_ids=bm, instance_names=inst, material_names=mat, compression="zip", half=True)
    path = str(tmp_path / "api.exr")
    ctx.write_layers_exr(path, w, h, dev[0].ptr, codes="dynamic", **kw)
    assert open(path, "rb").read() == data
    ctx.write_layers_exr(path, w, h, dev[0].ptr, **kw)
    assert open(path, "rb").read() == plain["refrun_layers_0000.exr"]


# ---- the CPU tier's run of the above ------------------------------------------------------------------------------------------------------------
def test_dynamic_kernels_on_the_emulation():
    """CPU tier: this file's GPU tests run by a child pytest against the emulation builds (tests/emu/Makefile.exr: exr_zip.hip unmodified on the HIP-on-CPU shim) —
    every one of them runs and passes there, none skipped (the drop-in test where the drop-in program is built)."""
    run_gpu_tests_on_emulation(__file__, 9, passed_without_dropin=8,extra_env={"CRX_LIB": os.path.join(EMU_DIR, "libcray_hip_exr_emu.so")},
                               make_targets=("libcray_hip_emu.so", "-f Makefile.exr"), dropin_libs=("libcray_hip_exr.so",))

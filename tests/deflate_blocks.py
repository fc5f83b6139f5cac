"""What tests/test_exr_dynamic.py measures deflate streams and prefix codes with, written from RFC 1951 alone (pure Python, no test lives here):
a walker that inflates a raw deflate stream itself and reports every block — its type, the three code-length vectors of a dynamic block, its tokens and the
bytes it spans —, a package-merge reference for optimal length-limited code lengths, and Huffman's lengths by the two-queue method (a leaf before a node of
equal weight: the optimal tree of least depth). Both are anchored in tests/test_exr_dynamic.py: the walker against zlib.decompress on streams host zlib makes,
package-merge by its Kraft sum and by Huffman's cost where the limit does not bind."""
from fractions import Fraction

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30          # (the two codes 30 and 31 never occur)


class _Bits:
    def __init__(self, data):
        self.data, self.at = bytes(data), 0          # at: in bits

    def peek(self, n):
        """the next n bits, the first the least significant; zeros behind the end of the data"""
        first = self.at >> 3
        return (int.from_bytes(self.data[first:first + 4], "little") >> (self.at & 7)) & ((1 << n) - 1)          # n <= 16: 7 + 16 bits lie in 3 bytes

    def take(self, n):
        v = self.peek(n)
        self.at += n
        assert self.at <= 8 * len(self.data), "the stream ends inside a block"
        return v


def canonical(lengths):
    """The canonical code (RFC 1951, 3.2.2) for a vector of lengths as a decoding table: (the longest length m, a list of 2^m entries indexed by the next m bits of
    the stream as they come — a Huffman code enters most significant bit first, so its bits are the index's low bits, reversed — holding (symbol, length), or None
    where no code begins so: an incomplete code)"""
    count = [0] * 16
    for length in lengths:
        count[length] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    longest = max(max(lengths), 1)
    table = [None] * (1 << longest)
    for sym, length in enumerate(lengths):
        if length:
            code = nxt[length]
            nxt[length] += 1
            assert code < 1 << length, "an oversubscribed code"
            first = int(format(code, f"0{length}b")[::-1], 2)
            table[first::1 << length] = [(sym, length)] * (1 << (longest - length))
    return longest, table


def _symbol(bits, code):
    entry = code[1][bits.peek(code[0])]
    assert entry is not None, "a code no symbol has"
    bits.take(entry[1])
    return entry[0]


def kraft(lengths):
    """the Kraft sum of the used symbols, exactly"""
    return sum((Fraction(1, 2 ** b) for b in lengths if b), Fraction(0))


def walk(data):
    """A raw deflate stream (no zlib header) -> (the bytes it inflates to, its blocks, the bytes of `data` it spans). A block: btype 0 / 1 / 2, final, span (first
    byte, one past the last byte it touches), literals and matches (token counts), distances (the set of distance symbols used), stored (bytes of a stored block),
    and for btype 2 the lengths `lit` [HLIT], `dist` [HDIST] and `cl` [19, by symbol], with hclen."""
    bits, out, blocks = _Bits(data), bytearray(), []
    while True:
        first = bits.at
        final, btype = bits.take(1), bits.take(2)
        assert btype != 3, "BTYPE 11"
        block = {"btype": btype, "final": final, "literals": 0, "matches": 0, "distances": set(), "stored": 0}
        if btype == 0:
            bits.at = (bits.at + 7) & ~7
            n, inverse = bits.take(16), bits.take(16)
            assert n ^ inverse == 0xFFFF, "LEN and NLEN"
            start = bits.at >> 3
            assert start + n <= len(data)
            out += data[start:start + n]
            bits.at += 8 * n
            block["stored"] = n
        else:
            if btype == 1:
                lit, dist = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                assert hlit <= 286 and hdist <= 30
                cl = [0] * 19
                for j in range(hclen):
                    cl[CL_ORDER[j]] = bits.take(3)
                assert kraft(cl) == 1, "the code-length code must be complete"
                table, seq = canonical(cl), []
                while len(seq) < hlit + hdist:
                    s = _symbol(bits, table)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        assert seq, "a repeat with nothing before it"
                        seq += [seq[-1]] * (3 + bits.take(2))
                    else:
                        seq += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(seq) == hlit + hdist, "a run past the end of the lengths"
                lit, dist = seq[:hlit], seq[hlit:]
                assert lit[256], "no end of block"
                for name, v in (("lit/len", lit), ("distance", dist)):          # what zlib's inflate_table accepts
                    used = [b for b in v if b]
                    assert kraft(v) == 1 or used == [1] or (name == "distance" and not used), f"an incomplete {name} code"
                block.update(lit=lit, dist=dist, cl=cl, hclen=hclen)
            lt, dt = canonical(lit), canonical(dist)
            while True:
                s = _symbol(bits, lt)
                if s < 256:
                    out.append(s)
                    block["literals"] += 1
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    d = _symbol(bits, dt)
                    assert d < 30
                    distance = DIST_BASE[d] + bits.take(DIST_EXTRA[d])
                    assert distance <= len(out), "a distance before the start"
                    for _ in range(length):
                        out.append(out[-distance])
                    block["matches"] += 1
                    block["distances"].add(d)
        block["span"] = (first >> 3, (bits.at + 7) >> 3)
        blocks.append(block)
        if final:
            return bytes(out), blocks, (bits.at + 7) >> 3


def walk_zlib(data):
    """walk() of a zlib stream: the header 78 01 in front, the Adler-32 behind (not checked here: zlib.decompress does that in the tests)"""
    assert data[:2] == b"\x78\x01"
    out, blocks, used = walk(data[2:-4])
    assert used == len(data) - 6, "bytes between the last block and the trailer"
    return out, blocks


# ---- prefix codes ------------------------------------------------------------------------------------------------------------------------------
def huffman_lengths(freq):
    """Huffman's code lengths, unlimited, by two queues — the leaves sorted by (count, symbol) and the nodes in the order they were made —, a leaf before a node of
    equal weight: among the optimal trees the one of least depth. One used symbol gets length 1."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    lengths, n = [0] * len(freq), len(used)
    if n == 1:
        lengths[used[0][1]] = 1
    if n < 2:
        return lengths
    weight, parent_leaf, parent_node, i, j = [], [0] * n, [0] * (n - 1), 0, 0
    for m in range(n - 1):
        w = 0
        for _ in range(2):
            if i < n and (j >= m or used[i][0] <= weight[j]):
                w += used[i][0]
                parent_leaf[i] = m
                i += 1
            else:
                w += weight[j]
                parent_node[j] = m
                j += 1
        weight.append(w)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[parent_node[k]] + 1
    for k, (_, s) in enumerate(used):
        lengths[s] = depth[parent_leaf[k]] + 1
    return lengths


def package_merge(freq, limit):
    """Optimal code lengths none longer than `limit` (Larmore and Hirschberg's package-merge): `limit` rounds of pairing up the cheapest items of the last list
    and merging the pairs with the leaves; a symbol's length is how often it occurs in the first 2 n - 2 items of the last list. One used symbol gets length 1."""
    leaves = sorted((f, s) for s, f in enumerate(freq) if f)
    lengths, n = [0] * len(freq), len(leaves)
    if n == 1:
        lengths[leaves[0][1]] = 1
    if n < 2:
        return lengths
    assert n <= 2 ** limit
    items = [(f, (s,)) for f, s in leaves]
    current = items
    for _ in range(limit - 1):
        packages = [(current[k][0] + current[k + 1][0], current[k][1] + current[k + 1][1]) for k in range(0, len(current) - 1, 2)]
        current = sorted(items + packages, key=lambda item: item[0])
    for _, symbols in current[:2 * n - 2]:
        for s in symbols:
            lengths[s] += 1
    return lengths


def cost(freq, lengths):
    return sum(int(f) * int(b) for f, b in zip(freq, lengths))

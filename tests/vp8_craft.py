"""vp8_craft.py — lossy WebP files made field by field: a bool *encoder*, a writer of
the VP8 key-frame header, the per-MB modes and the tokens, and the RIFF container.

Pillow cannot set these things.  Checked here (Pillow 12 / libwebp 1.6, quality 0..100,
method 0 / 4 / 6): every file it writes has one partition, the normal filter,
sharpness 0, no loop-filter deltas, version 0, and segmentation with a map except at
quality 100 and in tiny images.  Everything else of the format the tests get from here.

frame(w, h, mbs, **header) -> the VP8 chunk's payload; simple(payload) / extended(payload,
...) wrap it.  An MB is a dict: ymode (0 DC, 1 TM, 2 V, 3 H, 4 B_PRED), bmodes (16, for
B_PRED), uvmode, segment, skip, and levels: 25 lists of 16 quantised levels in scan
(zigzag) order: 16 luma blocks, 4 U, 4 V, then the Y2 block (used unless B_PRED).
"""
import ref_vp8 as R

B_PRED = 4


class BoolEnc:
    """The arithmetic coder of RFC 6386 section 7, the interval's low end kept as one integer."""

    def __init__(self):
        self.low, self.range, self.k = 0, 255, 0

    def put(self, bit, prob=128):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            self.low <<= 1
            self.k += 1

    def bits(self, v, n):
        for i in reversed(range(n)):
            self.put((v >> i) & 1)

    def signed(self, v, n):
        self.bits(abs(v), n)
        self.put(1 if v < 0 else 0)

    def opt_signed(self, v, n):
        """None: the flag says absent; a number (0 too): present."""
        if v is None:
            self.put(0)
        else:
            self.put(1)
            self.signed(v, n)

    def finish(self, pad=4):
        total = 8 + self.k
        nbytes = (total + 7) // 8
        return (self.low << (nbytes * 8 - total)).to_bytes(nbytes, "big") + b"\0" * pad


def _P(probs, typ, n, ctx):
    return probs[((typ * 8 + R.BANDS[n]) * 3 + ctx) * 11:][:11]


def put_coeffs(e, probs, typ, ctx, lv, first):
    """The tokens of one block (levels lv in scan order) from position `first`; returns what the decoder's
    GetCoeffs returns: 1 + the last non-zero position, or `first` for an empty block."""
    last = max([i for i in range(first, 16) if lv[i]], default=-1)
    n, p = first, _P(probs, typ, first, ctx)
    while n < 16:
        if n > last:
            e.put(0, p[0])
            return n
        e.put(1, p[0])
        while lv[n] == 0:
            e.put(0, p[1])
            n += 1
            p = _P(probs, typ, n, 0)
        e.put(1, p[1])
        v = abs(lv[n])
        if v == 1:
            e.put(0, p[2])
            nc = 1
        else:
            e.put(1, p[2])
            nc = 2
            if v <= 4:
                e.put(0, p[3])
                if v == 2:
                    e.put(0, p[4])
                else:
                    e.put(1, p[4])
                    e.put(v == 4, p[5])
            elif v <= 10:
                e.put(1, p[3])
                e.put(0, p[6])
                if v <= 6:
                    e.put(0, p[7])
                    e.put(v == 6, 159)
                else:
                    e.put(1, p[7])
                    e.put((v - 7) >> 1, 165)
                    e.put((v - 7) & 1, 145)
            else:
                e.put(1, p[3])
                e.put(1, p[6])
                cat = 0 if v <= 18 else 1 if v <= 34 else 2 if v <= 66 else 3
                assert v <= 2114
                e.put(cat >> 1, p[8])
                e.put(cat & 1, p[9 + (cat >> 1)])
                extra, tab = v - 3 - (8 << cat), R.CAT[cat]
                for i, pr in enumerate(tab):
                    e.put((extra >> (len(tab) - 1 - i)) & 1, pr)
        e.put(1 if lv[n] < 0 else 0, 128)
        n += 1
        p = _P(probs, typ, n, nc)
    return 16


def frame(w, h, mbs, version=0, show=1, key=1, start=b"\x9d\x01\x2a", colorspace=0, clamp=0, seg=None, simple=0,
          level=0, sharp=0, lf=None, nparts=1, base_q=40, dq=(None,) * 5, updates=None, skip_prob=None,
          part0_size=None, part_sizes=None, xscale=0, yscale=0, pad=4):
    """seg: dict(map=bool, data=None | dict(abs=0/1, q=[4 x None|int], f=[4 x None|int]), probs=[3 x None|int]).
    lf: dict(update=bool, ref=[4 x None|int], mode=[4 x None|int]).  updates: {probability index: value}.
    part0_size / part_sizes: what the headers claim, where the truth is not wanted."""
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    assert len(mbs) == mbw * mbh
    e = BoolEnc()
    e.put(colorspace)
    e.put(clamp)
    seg_p = [255] * 3
    e.put(1 if seg else 0)
    if seg:
        e.put(1 if seg.get("map") else 0)
        data = seg.get("data")
        e.put(1 if data else 0)
        if data:
            e.put(data["abs"])
            for v in data["q"]:
                e.opt_signed(v, 7)
            for v in data["f"]:
                e.opt_signed(v, 6)
        if seg.get("map"):
            for i, v in enumerate(seg.get("probs", [None] * 3)):
                e.put(0 if v is None else 1)
                if v is not None:
                    e.bits(v, 8)
                    seg_p[i] = v
    e.put(simple)
    e.bits(level, 6)
    e.bits(sharp, 3)
    e.put(1 if lf else 0)
    if lf:
        e.put(1 if lf.get("update") else 0)
        if lf.get("update"):
            for v in lf["ref"]:
                e.opt_signed(v, 6)
            for v in lf["mode"]:
                e.opt_signed(v, 6)
    e.bits({1: 0, 2: 1, 4: 2, 8: 3}[nparts], 2)
    e.bits(base_q, 7)
    for v in dq:
        e.opt_signed(v, 4)
    e.put(0)  # refresh entropy probabilities
    probs = list(R.COEF0)
    updates = updates or {}
    for i in range(1056):
        if i in updates:
            e.put(1, R.UPD[i])
            e.bits(updates[i], 8)
            probs[i] = updates[i]
        else:
            e.put(0, R.UPD[i])
    e.put(0 if skip_prob is None else 1)
    if skip_prob is not None:
        e.bits(skip_prob, 8)
    toks = [BoolEnc() for _ in range(nparts)]
    top_modes, top_nz, top_dc = [0] * (4 * mbw), [0] * mbw, [0] * mbw
    for my in range(mbh):
        t = toks[my & (nparts - 1)]
        left_modes, left_nz, left_dc = [0] * 4, 0, 0
        for mx in range(mbw):
            mb = mbs[my * mbw + mx]
            s = mb.get("segment", 0)
            if seg and seg.get("map"):
                e.put(s >> 1, seg_p[0])
                e.put(s & 1, seg_p[2] if s >> 1 else seg_p[1])
            skip = mb.get("skip", 0) if skip_prob is not None else 0
            if skip_prob is not None:
                e.put(skip, skip_prob)
            ym = mb["ymode"]
            i4 = ym == B_PRED
            e.put(0 if i4 else 1, 145)
            if not i4:
                e.put(1 if ym in (1, 3) else 0, 156)
                if ym in (1, 3):
                    e.put(1 if ym == 1 else 0, 128)
                else:
                    e.put(1 if ym == 2 else 0, 163)
                top_modes[4 * mx:4 * mx + 4] = [ym] * 4
                left_modes = [ym] * 4
            else:
                for yy in range(4):
                    m = left_modes[yy]
                    for xx in range(4):
                        pr = R.BMODES[(top_modes[4 * mx + xx] * 10 + m) * 9:][:9]
                        m = mb["bmodes"][4 * yy + xx]
                        path = _tree_path(m)
                        for node, bit in path:
                            e.put(bit, pr[node])
                        top_modes[4 * mx + xx] = m
                    left_modes[yy] = m
            uv = mb.get("uvmode", 0)
            e.put(0 if uv == 0 else 1, 142)
            if uv:
                e.put(0 if uv == 2 else 1, 114)
                if uv != 2:
                    e.put(1 if uv == 1 else 0, 183)
            if skip:
                left_nz = top_nz[mx] = 0
                if not i4:
                    left_dc = top_dc[mx] = 0
                continue
            lv = mb["levels"]
            if not i4:
                nz = put_coeffs(t, probs, 1, top_dc[mx] + left_dc, lv[24], 0)
                top_dc[mx] = left_dc = 1 if nz > 0 else 0
                first, typ = 1, 0
            else:
                first, typ = 0, 3
            tnz, lnz = top_nz[mx] & 15, left_nz & 15
            for yy in range(4):
                l = lnz & 1
                for xx in range(4):
                    nz = put_coeffs(t, probs, typ, l + (tnz & 1), lv[4 * yy + xx], first)
                    l = 1 if nz > first else 0
                    tnz = (tnz >> 1) | (l << 7)
                tnz >>= 4
                lnz = (lnz >> 1) | (l << 7)
            out_t, out_l = tnz, lnz >> 4
            for ch in (0, 2):
                tnz, lnz = top_nz[mx] >> (4 + ch), left_nz >> (4 + ch)
                for yy in range(2):
                    l = lnz & 1
                    for xx in range(2):
                        nz = put_coeffs(t, probs, 2, l + (tnz & 1), lv[16 + 2 * ch + 2 * yy + xx], 0)
                        l = 1 if nz > 0 else 0
                        tnz = (tnz >> 1) | (l << 3)
                    tnz >>= 2
                    lnz = (lnz >> 1) | (l << 5)
                out_t |= (tnz << 4) << ch
                out_l |= (lnz & 0xf0) << ch
            top_nz[mx], left_nz = out_t & 0xff, out_l & 0xff
    p0 = e.finish(pad)
    parts = [t.finish(pad) for t in toks]
    tag = (0 if key else 1) | (version << 1) | (show << 4) | ((len(p0) if part0_size is None else part0_size) << 5)
    out = tag.to_bytes(3, "little") + start + (w | (xscale << 14)).to_bytes(2, "little") + (h | (yscale << 14)).to_bytes(2, "little")
    out += p0
    for i, p in enumerate(parts[:-1]):
        out += (len(p) if part_sizes is None else part_sizes[i]).to_bytes(3, "little")
    return out + b"".join(parts)


def _tree_path(mode):
    """[(probability index, bit)] from the root of the sub-block mode tree to leaf `mode`."""
    def walk(i, path):
        for bit in (0, 1):
            nxt = R.BMODE_TREE[2 * i + bit]
            here = path + [(i, bit)]
            if nxt > 0:
                r = walk(nxt, here)
                if r:
                    return r
            elif -nxt == mode:
                return here
        return None
    r = walk(0, [])
    assert r is not None, mode
    return r


def chunk(cc, body):
    return cc + len(body).to_bytes(4, "little") + body + (b"\0" if len(body) & 1 else b"")


def riff(chunks):
    body = b"WEBP" + b"".join(chunks)
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def simple(payload):
    return riff([chunk(b"VP8 ", payload)])


def extended(payload, w, h, flags=0, before=(), after=()):
    """VP8X (flags: 0x20 ICC, 0x10 alpha, 0x08 EXIF, 0x04 XMP, 0x02 animation), chunks before and after the image."""
    x = bytes([flags, 0, 0, 0]) + (w - 1).to_bytes(3, "little") + (h - 1).to_bytes(3, "little")
    return riff([chunk(b"VP8X", x)] + list(before) + [chunk(b"VP8 ", payload)] + list(after))


def frame_info(data):
    """What a Pillow-made file chose: dict(parts, simple, sharp, lf_delta, version, seg, seg_map)."""
    h = R.parse(data)
    assert h["status"] == R.OK
    off = h["off"]
    br = R.BoolDec(data, off + 10, off + 10 + h["part0"])
    br.get(2)
    seg = br.get(1)
    seg_map = 0
    if seg:
        seg_map = br.get(1)
        if br.get(1):
            br.get(1)
            for n in (7, 6):
                for _ in range(4):
                    if br.get(1):
                        br.signed(n)
        if seg_map:
            for _ in range(3):
                if br.get(1):
                    br.get(8)
    simple_f, _, sharp = br.get(1), br.get(6), br.get(3)
    lf = br.get(1)
    if lf and br.get(1):
        for _ in range(8):
            if br.get(1):
                br.signed(6)
    return dict(parts=1 << br.get(2), simple=simple_f, sharp=sharp, lf_delta=lf, version=(data[off] >> 1) & 7, seg=seg,
                seg_map=seg_map)

"""The corpus the all-formats tests share (test_all_formats_cpu.py, test_gpu_all_formats.py): members of every
format and form the library decodes behind a context option, none larger than 128 x 128 and no two neighbours of one
size, each with the decode of something that is not this library; the failing files with the status each must give;
and larger members of every family for the batch under a device budget.  Everything is built with the crafting and
case modules the families' own tests use, seeded, so every process sees the same bytes."""
import functools
import io

import numpy as np
from PIL import Image

import alph_cases
import alph_craft
import bmp_cases
import bmp_craft
import gif_cases
import gif_craft
import ref_alph
import ref_bmp
import ref_gif
import ref_vp8
import ref_webp
import tiff16_craft as S
import tiff_craft as T
import tiff_deflate_craft as D
import vp8_cases
import webp_cases
from datago_amd import synth
from oracle import oracle as O

FAMILIES = ["jpeg", "png", "gif", "webp", "bmp", "tiff", "tiff_deflate", "tiff16"]
# every format option switched on (dg_ctx_set_option names)
ALL_ON = dict(png16=1, gif=1, webp=1, webp_lossy=1, webp_alpha=1, bmp=1, tiff=1, tiff_deflate=1, tiff16=1,
              jpeg_cmyk=1, jpeg_h1v2=1, jpeg_multiscan=1)
MAX_SIDE = 128
# members a test must find by name
BMP_NO_INDEX = "bmp 24-bit"
CORRUPT, UNSUPPORTED = "CORRUPT", "UNSUPPORTED"


def _oracle(data):
    st, arr = O.decode_any(data)
    assert st == 0, st
    return arr


def _pillow(data):
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a.reshape(a.shape[0], a.shape[1], -1)


def _hwc(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _jpeg():
    import test_gpu_jpeg_cmyk as JC
    import test_gpu_jpeg_h1v2 as JH
    import test_gpu_jpeg_multiscan as JM
    plain = [("gray", synth.make_jpeg(1, 90, 61, 85, gray=True)),
             ("4:4:4", synth.make_jpeg(2, 77, 64, 90, "4:4:4")),
             ("4:2:0 restart", synth.make_jpeg(4, 95, 63, 88, "4:2:0", restart_marker_rows=1)),
             ("4:2:2", synth.make_jpeg(9, 64, 96, 75, "4:2:2")),
             ("progressive", synth.make_jpeg(5, 93, 58, 90, "4:2:0", progressive=True))]
    out = [("jpeg", "jpeg " + label, d, _oracle(d), 8) for label, d in plain]
    crafted = [("4:4:0", JH.Case("440", 37, 29, seed=3, restart=3)), ("cmyk", JC.Case("cmyk_444", 0, 45, 31, seed=3)),
               ("ycck", JC.Case("ycck_420", 2, 52, 39, seed=4, restart=1)),
               ("multiscan", JM.Case("420", 41, 27, [[0], [1, 2]], seed=3, restart=2))]
    return out + [("jpeg", "jpeg " + label, c.data, _hwc(c.ref(0)), 8) for label, c in crafted]


def _png():
    rng = np.random.default_rng(4242)
    noise = rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    plain = [("RGB", synth.make_png(6, 83, 59, "RGB")), ("palette", synth.make_png(7, 71, 64, "P8")),
             ("RGBA Adam7", synth.make_png(8, 61, 47, "RGBA", interlace=True)),
             # incompressible: > 12 KiB of IDAT, three chunks at inf_chunk 4096
             ("noise chunked", synth.encode_png(noise.reshape(64, 64 * 3), 64, 64, 8, 2, 3, rng, filters="none"))]
    out = [("png", "png " + label, d, _oracle(d), 8) for label, d in plain]
    g16 = rng.integers(0, 65536, size=(50, 70, 1), dtype=np.uint16)
    c16 = rng.integers(0, 65536, size=(61, 45, 3), dtype=np.uint16)
    return out + [("png", "png gray16", synth.encode_png16(g16, 0, rng), g16, 16),
                  ("png", "png rgb16", synth.encode_png16(c16, 2, rng), c16, 16)]


def _ref_gif(data):
    st, why, rgba, _ = ref_gif.decode(data)
    assert st == ref_gif.OK, why
    return rgba


def _gif():
    G, C = gif_craft, gif_cases
    pal = G.palette(32, 61)
    files = [("global table", G.gif(90, 50, C.photo(50, 90, 32, 62), 5, gct=pal)),
             ("local table", G.gif(45, 31, C.photo(31, 45, 8, 63), 3, gct=G.palette(8, 21), lct=G.palette(8, 23))),
             ("interlaced", G.gif(19, 67, C.photo(67, 19, 32, 64), 5, gct=pal, interlace=True)),
             ("transparent index", G.gif(73, 41, C.photo(41, 73, 32, 65), 5, gct=pal, before=[G.gce(transparent=7)]))]
    return [("gif", "gif " + label, d, _ref_gif(d), 8) for label, d in files]


def _ref_webp(data):
    r = ref_webp.decode(data)
    assert r.status == "OK", r.why
    return r.pixels


def _ref_vp8(data):
    r = ref_vp8.decode(data)
    assert r.status == ref_vp8.OK, r.why
    return np.frombuffer(r.rgb, np.uint8).reshape(r.height, r.width, 3)


def _ref_alph(data):
    r = ref_alph.decode(data)
    assert r.status == ref_alph.OK, r.why
    return np.frombuffer(r.pixels, np.uint8).reshape(r.height, r.width, r.channels)


def _webp():
    lossless, lossy = dict(webp_cases.crafted_cases()), dict(vp8_cases.crafted_cases())
    photo = next((n, d) for n, d in webp_cases.pillow_cases() if n.startswith("photo_127x65"))
    alph = dict(alph_cases.crafted_cases())
    out = [("webp", "webp lossless " + n, d, _ref_webp(d), 8) for n, d in
           [("index_2colours_33x4", lossless["index_2colours_33x4"]), ("predictor_mixed_modes", lossless["predictor_mixed_modes"]),
            ("cache_bits11", lossless["cache_bits11"]), photo]]
    out += [("webp", "webp lossy " + n, d, _ref_vp8(d), 8) for n, d in
            [("seg_delta", lossy["seg_delta"]), ("parts4_20x77", lossy["parts4_20x77"]),
             ("photo_17x33", dict(vp8_cases.pillow_cases())["photo_17x33"])]]
    out += [("webp", "webp alpha " + n, d, _ref_alph(d), 8) for n, d in
            [("raw_f3_63x64", alph["raw_f3_63x64"]), ("vp8l_transforms_f2_65x65", alph["vp8l_transforms_f2_65x65"]),
             ("pillow blob", dict(alph_cases.pillow_cases())["blob"])]]
    return out


def _ref_bmp(data):
    st, why, pix, _ = ref_bmp.decode(data)
    assert st == ref_bmp.OK, why
    return pix


def _bmp():
    G, C = bmp_craft, bmp_cases
    ph = C.photo(50, 77, 256, 63)
    files = [(BMP_NO_INDEX, G.bmp(101, 37, 24, C.rgb(37, 101, 61))),
             ("bmp RLE8", G.bmp(77, 50, 8, data=G.rle_bytes(G.rle_commands(ph, False, "mixed")), compression=G.RLE8,
                                pal=G.palette(256, 64))),
             ("bmp 32-bit masks alpha", G.bmp(58, 66, 32, C.rgb(66, 58, 62, 4), top_down=True, compression=G.BITFIELDS,
                                              masks=G.MASKS32[5], header=108)),
             ("bmp 8-bit palette bottom-up", G.bmp(43, 29, 8, C.noise(29, 43, 256, 65), pal=G.palette(256, 66)))]
    return [("bmp", label, d, _ref_bmp(d), 8) for label, d in files]


def _runs(a):
    a = a.copy()
    a[a.shape[0] // 4:a.shape[0] // 2] = a[0, 0]  # something for PackBits, LZW and Deflate to find
    return a


def _tiff():
    """8-bit TIFFs.  (file, the array it was made from); the reference is Pillow's decode."""
    g1, g2 = T.noise(50, 83, 1, 31), _runs(T.noise(44, 61, 1, 32))
    la, n3, n4 = _runs(T.noise(57, 39, 2, 33)), _runs(T.noise(70, 97, 3, 34)), _runs(T.noise(75, 66, 4, 35))
    # one tile of 144 x 128 RGBA samples decodes to 73,728 bytes: over what k_tiff_lzw keeps in LDS
    big = _runs(T.noise(128, 121, 4, 36))
    files = [("raw gray MM", T.tiff(g1, be=True), g1), ("WhiteIsZero lzw", T.tiff(g2, photo=0, comp=5), 255 - g2),
             ("La8 packbits", T.tiff(la, comp=32773), la), ("Rgb8 lzw pred rps 7", T.tiff(n3, comp=5, pred=2, rps=7), n3),
             ("Rgba8 lzw pred tiles", T.tiff(n4, comp=5, pred=2, tile=(32, 32)), n4),
             ("Rgba8 lzw pred segment over LDS", T.tiff(big, comp=5, pred=2, tile=(144, 128)), big)]
    return [("tiff", "tiff " + label, d, _pillow(d), 8, _hwc(pix)) for label, d, pix in files]


def _tiff_deflate():
    a, b = _runs(T.noise(53, 88, 3, 41)), _runs(T.noise(72, 59, 3, 42))
    files = [("dynamic", T.tiff(a, comp=8, pack=D.z()), a), ("stored pred", T.tiff(b, comp=8, pred=2, pack=D.z(0)), b)]
    return [("tiff_deflate", "tiff_deflate " + label, d, _pillow(d), 8, _hwc(pix)) for label, d, pix in files]


def _tiff16():
    files = [S.tiff16("gray16 II lzw pred", S.noise16(47, 85, 1, 51), comp=5, pred=2),
             S.tiff16("La16 packbits", S.noise16(63, 38, 2, 52), comp=32773, rps=9),
             S.tiff16("Rgb16 MM lzw pred", S.noise16(54, 71, 3, 53), be=True, comp=5, pred=2, rps=9),
             S.tiff16("Rgba16 tiles lzw pred", S.noise16(69, 60, 4, 54), tile=(16, 16), comp=5, pred=2),
             # one strip of 128 x 128 x 4 samples: 131,072 bytes, twice what k_tiff_inflate keeps in LDS
             S.tiff16("Rgba16 deflate pred strip over LDS", S.noise16(128, 128, 4, 55), comp=8, pred=2, pack=D.z())]
    return [("tiff16", "tiff16 " + label, d, _hwc(pix), 16) for label, d, pix in files]


@functools.lru_cache(maxsize=None)
def _built():
    out = []
    for fn in (_jpeg, _png, _gif, _webp, _bmp, _tiff, _tiff_deflate, _tiff16):
        out += fn()
    return out


def corpus():
    """[(family, label, file, reference, bits)]: reference is H x W x C, uint8, or uint16 where bits is 16."""
    return [m[:5] for m in _built()]


def sources():
    """{label: the array a file was made from} for the members whose reference is Pillow's decode."""
    return {m[1]: m[5] for m in _built() if len(m) > 5}


@functools.lru_cache(maxsize=None)
def bad():
    """[(label, file, status, family or None)]: files that fail, with the status each must give; family names the
    format of a refusal that a kernel meets at completion, between whose good members it goes."""
    head = synth.make_jpeg(10, 80, 60, 90)
    gif, webp = {r[0]: r for r in gif_cases.refusals()}, {r[0]: r for r in webp_cases.refusals()}
    bmp, vp8 = {r[0]: r for r in bmp_cases.refusals()}, {r[0]: r for r in vp8_cases.refusals()}
    tiff, tinf = {r[0]: r for r in T.refusals()}, dict(D.refusals())
    assert vp8["tokens cut"][4] and tiff["stream: short LZW"][2] and not tiff["BigTIFF"][2]
    return [("bad jpeg truncated header", head[:head.index(b"\xff\xc0") + 6], CORRUPT, None),
            ("bad garbage", np.random.default_rng(4242).integers(0, 256, size=700, dtype=np.uint8).tobytes(), CORRUPT, None),
            ("bad gif header", gif["ends in the global table"][1], CORRUPT, None),
            ("bad webp header", webp["bad_signature"][1], CORRUPT, None),
            ("bad bmp header", bmp["16-bit 555"][1], UNSUPPORTED, None),
            ("bad tiff header", tiff["BigTIFF"][1], UNSUPPORTED, None),
            ("bad tiff stream: short LZW", tiff["stream: short LZW"][1], CORRUPT, "tiff"),
            ("bad tiff_deflate stream: wrong Adler-32", tinf["wrong Adler-32"], CORRUPT, "tiff_deflate"),
            ("bad webp stream: tokens cut", vp8["tokens cut"][1], CORRUPT, "webp"),
            ("bad gif stream: data runs out", gif["data runs out"][1], UNSUPPORTED, "gif"),
            ("bad bmp stream: RLE8 data ends early", bmp["RLE8 data ends early"][1], UNSUPPORTED, "bmp")]


def order():
    """The interleaved batch [(label, file, family or None for a bad one)]: a bad file first, bad ones between the
    families, one near the end, and each stream-level refusal between two good files of its own format."""
    good, bads = corpus(), list(bad())
    header = [b for b in bads if b[3] is None]
    out = [(header[0][0], header[0][1], None)]
    for k, fam in enumerate(FAMILIES):
        members = [(m[1], m[2], fam) for m in good if m[0] == fam]
        for b in (b for b in bads if b[3] == fam):
            members.insert(len(members) // 2, (b[0], b[1], None))
        if fam == FAMILIES[-1]:  # the last header-level refusal: two good files before the end
            members.insert(len(members) - 2, (header[-1][0], header[-1][1], None))
        out += members
        if 1 + k < len(header) - 1:
            out.append((header[1 + k][0], header[1 + k][1], None))
    assert len(out) == len(good) + len(bads)
    return out


def rotations():
    """[(name, batch)]: the order as it stands (a bad file first), and turned so that each family's first member
    stands first."""
    base = order()
    out = [("bad first", base)]
    for fam in FAMILIES:
        k = next(i for i, m in enumerate(base) if m[2] == fam)
        out.append((fam + " first", base[k:] + base[:k]))
    return out


def rotated(batch, label):
    """`batch` turned so that the member `label` stands first."""
    k = next(i for i, m in enumerate(batch) if m[0] == label)
    return batch[k:] + batch[:k]


# ------------------------------------------------------------------ larger members, for the batch under a budget

def _photo(seed, h, w, c=3):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([128 + 100 * np.sin(x / (7.0 + k) + y / 11.0) for k in range(c)], -1)
    return np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def large(rounds=3):
    """[(family, label, file)]: every family once per round, 400 to 700 px a side, from the same builders."""
    G, B = gif_craft, bmp_craft
    out = []
    for r in range(rounds):
        w, h = 700 - 90 * r, 400 + 70 * r
        s = 900 + 10 * r
        deep = np.random.default_rng(s).integers(0, 65536, size=(h, w, 3), dtype=np.uint16)
        deep[h // 4:h // 2] = deep[0, 0]
        out += [("jpeg", "large jpeg %d" % r, synth.make_jpeg(s, w, h, 90, ("4:2:0", "4:4:4", "4:2:2")[r % 3])),
                ("png", "large png %d" % r, synth.make_png(s + 1, h, w, ("RGBA", "RGB", "P8")[r % 3])),
                ("gif", "large gif %d" % r, G.gif(w, h, gif_cases.photo(h, w, 32, s + 2), 5, gct=G.palette(32, 61))),
                ("webp", "large webp %d" % r, (webp_cases._save(_photo(s + 3, h, w), 3, 50), vp8_cases.save(_photo(s + 3, h, w), 75, 4),
                                               alph_craft.save(_photo(s + 3, h, w, 4), quality=75))[r % 3]),
                ("bmp", "large bmp %d" % r, B.bmp(h, w, 24, bmp_cases.rgb(w, h, s + 4))),
                ("tiff", "large tiff %d" % r, T.tiff(_photo(s + 5, h, w, (3, 4, 1)[r % 3]), comp=32773, rps=16)),
                ("tiff_deflate", "large tiff_deflate %d" % r, T.tiff(_photo(s + 6, w, h), comp=8, pred=2, rps=32, pack=D.z())),
                ("tiff16", "large tiff16 %d" % r, S.tiff16("", deep, comp=32773, rps=16, be=r % 2 == 1)[1])]
    return out

"""The JPEG re-encoder with per-image Huffman tables (context option
"jenc_optimize"; k_enc_hist and k_enc_tree of dg_enc.hip).  Inputs are
jenc_opt_cases.cases(): PNG files that decode losslessly to crafted pixels and
are encoded at their own size through a context without a transform, so each
8x8 block reaches the kernels as built.  test_jenc_opt_cpu.py proves on the
reference that the set reaches the rule's edges.

The claim, for any input on any path: the file with the option on equals
ref_jenc_opt.optimise(the file with the option off), and the latter equals
oracle.jpeg_encode's.  Every comparison is equality."""
import threading

import numpy as np
import pytest

import enc_cases as E
import jenc_opt_cases as C
import ref_jenc_opt as R

pytestmark = pytest.mark.gpu

FMT_PNG, FMT_JPEG = 0, 1
RESIZE = dict(crop_and_resize=True, default_image_size=512, downsampling_ratio=32, min_aspect_ratio=0.5,
              max_aspect_ratio=2.0)
CASES = C.cases()
BY_LABEL = {c[0]: c[1] for c in CASES}
_inputs = {}


def _lib():
    from datago_amd import _lib as L
    return L


def _ctx(optimize, quality=92, fmt=FMT_JPEG, **kw):
    return _lib().Context(0, pre_encode_images=True, encode_format=fmt, jpeg_quality=quality,
                          jenc_optimize=optimize, **kw)


def _input(label):
    if label not in _inputs:
        _inputs[label] = E.png_input(BY_LABEL[label])
    return _inputs[label]


def _same(got, exp, label):
    if got != exp:
        n = min(len(got), len(exp))
        at = next((i for i in range(n) if got[i] != exp[i]), n)
        raise AssertionError(f"{label}: {len(got)} bytes against the reference's {len(exp)}, first difference at "
                             f"byte {at}: {got[at:at + 8].hex()} / {exp[at:at + 8].hex()}")


def _files(ctx, datas, what="batch"):
    """One decode_batch; the surface of every result checked; returns the files."""
    out = []
    for i, (d, (st, enc, m)) in enumerate(zip(datas, ctx.decode_batch(datas))):
        assert st == 0, (what, i, _lib().last_error())
        got = enc.tobytes()
        assert m.is_encoded == 1 and m.channels == -1 and m.nbytes == len(got), (what, i)
        st, cap = ctx.output_size(d)
        assert st == 0 and m.nbytes <= cap, (what, i, m.nbytes, cap)
        assert got[:2] == b"\xff\xd8" and got[-2:] == b"\xff\xd9", (what, i)
        out.append(got)
    return out


def _header_len(data):
    return R.segments(data)[-1][2]


def _labels_at(quality):
    return [label for label, _, qs, _ in CASES if quality in qs]


def _shuffled(items, seed):
    return [items[i] for i in np.random.default_rng(seed).permutation(len(items))]


# ------------------------------------------------------------------ 1. bytes

@pytest.mark.parametrize("quality", C.QUALITIES)
def test_bytes(quality):
    labels = _shuffled(_labels_at(quality), quality)
    assert len(labels) >= 70 and ((C.LIMIT_LABEL in labels) == (quality == 50))
    datas = [_input(k) for k in labels]
    off = _files(_ctx(False, quality), datas, "option off")
    on = _files(_ctx(True, quality), datas, "option on")
    failed = []
    for label, a, b in zip(labels, off, on):
        _same(a, C.std_file(label, BY_LABEL[label], quality), f"{label} with the option off")
        tw = C.twin(label, BY_LABEL[label], quality)
        assert not tw.fallback and tw.file != a
        try:
            _same(b, tw.file, label)
            assert _header_len(b) <= _header_len(a) and len(b) < len(a)
        except AssertionError as err:
            failed.append((label, str(err)[:300]))
    assert not failed, f"{len(failed)} of {len(labels)} files differ; first: {failed[0]}"


# ------------------------------------------------------------------ 2. the option as a switch

def _handful():
    return ["flat_8x8_gray", "block_8x8_rgb", "partial_13x9_gray", "partial_13x9_rgb", "basis44_redcyan",
            "dc_alternate_gray", "b77_amp16_rgb", "noise_17x15", "noise_64x64_binary_rgb", "blocks_1025"]


def test_switch():
    L = _lib()
    labels = _handful()
    datas = [_input(k) for k in labels]
    std = [C.std_file(k, BY_LABEL[k], 92) for k in labels]
    opt = [C.twin(k, BY_LABEL[k], 92).file for k in labels]
    ctx = L.Context(0, pre_encode_images=True, encode_format=FMT_JPEG, jpeg_quality=92)
    for v, want in ((0, std), (1, opt), (0, std), (1, opt)):
        ctx.set_option("jenc_optimize", v)
        for label, g, w in zip(labels, _files(ctx, datas), want):
            _same(g, w, f"{label} with jenc_optimize = {v}")
    for bad in (-1, 2):
        with pytest.raises(L.DgError) as e:
            ctx.set_option("jenc_optimize", bad)
        assert e.value.status == L.DG_ERR_INVALID and "jenc_optimize" in L.last_error()
        assert str(bad) in L.last_error()
    for g, w in zip(_files(ctx, datas), opt):  # a rejected value changes nothing
        assert g == w


def test_png_encoding_untouched():
    datas = [_input(k) for k in _handful()]
    plain = _lib().Context(0, pre_encode_images=True, encode_format=FMT_PNG).decode_batch(datas)
    on = _ctx(True, fmt=FMT_PNG).decode_batch(datas)
    for (s0, e0, _), (s1, e1, _) in zip(plain, on):
        assert s0 == 0 and s1 == 0 and e0.tobytes() == e1.tobytes() and e0.tobytes()[:4] == b"\x89PNG"


def test_16_bit_stays_unsupported():
    from datago_amd import synth
    L = _lib()
    rng = np.random.default_rng(6200)
    deep = synth.encode_png16(rng.integers(0, 65536, (24, 40, 1)).astype(np.uint16), 0, rng)
    ctx = _ctx(True, png16=True)
    (st, _, _), (st8, enc, _) = ctx.decode_batch([deep, _input("block_8x8_rgb")])
    assert st == L.DG_ERR_UNSUPPORTED and st8 == 0
    assert enc.tobytes() == C.twin("block_8x8_rgb", BY_LABEL["block_8x8_rgb"], 92).file


def test_without_pre_encode_untouched():
    datas = [_input(k) for k in _handful()]
    a = _lib().Context(0).decode_batch(datas)
    ctx = _lib().Context(0)
    ctx.set_option("jenc_optimize", 1)
    for (s0, p0, m0), (s1, p1, m1) in zip(a, ctx.decode_batch(datas)):
        assert s0 == 0 and s1 == 0 and m1.is_encoded == 0 and np.array_equal(p0, p1)


# ------------------------------------------------------------------ 3. batch against alone

def test_batch_against_alone():
    """The histogram, the table region and the header length are per image: nothing leaks between the images of a
    batch, gray beside colour, a one-symbol table beside a limited one."""
    labels = ["flat_8x8_gray", "block_8x8_rgb", "partial_13x9_gray", "partial_13x9_rgb", C.LIMIT_LABEL, C.NOISE_LABEL,
              "flat128_c3", "noise_64x64_binary_gray"]
    datas = [_input(k) for k in labels]
    ctx = _ctx(True, 50)
    batch = _files(ctx, datas)
    for label, d, b in zip(labels, datas, batch):
        _same(b, C.twin(label, BY_LABEL[label], 50).file, label)
        alone, = _files(ctx, [d], label)
        assert alone == b, label


def _sources():
    from datago_amd import synth
    return [synth.make_jpeg(6300, 1000, 700, 90), synth.make_png(6301, 700, 900, "RGB"),
            synth.make_jpeg(6302, 640, 480, 85, gray=True), synth.make_png(6303, 333, 222, "RGBA"),
            synth.make_png(6304, 400, 300, "L")]


def test_resized_batch_against_alone():
    """JPEG and PNG sources resized to their 512 / 32 bucket beside the crafted arrays (resized too): each file
    equals the one the image gives alone and the twin of the same context's file without the option."""
    datas = _sources() + [_input(k) for k in ("flat_8x8_gray", "partial_13x9_rgb", C.NOISE_LABEL, C.LIMIT_LABEL)]
    on, off = _ctx(True, 92, **RESIZE), _ctx(False, 92, **RESIZE)
    batch, std = _files(on, datas), _files(off, datas)
    for i, (d, b, s) in enumerate(zip(datas, batch, std)):
        tw = R.optimise(s)
        assert not tw.fallback
        _same(b, tw.file, f"member {i}")
        assert _header_len(b) <= _header_len(s) and len(b) < len(s), i
        alone, = _files(on, [d], f"member {i} alone")
        assert alone == b, i


# ------------------------------------------------------------------ 4. paths

def _twelve():
    from datago_amd import synth
    datas = [synth.make_jpeg(6400 + i, 1024 - 40 * i, 768 + 16 * i, 90, ("4:2:0", "4:4:4")[i % 2]) for i in range(9)]
    datas.append(synth.make_jpeg(6410, 700, 500, 90, "4:2:0", progressive=True))  # the progressive aggregate
    datas.append(synth.make_png(6411, 900, 700, "RGB"))
    datas.append(synth.make_jpeg(6412, 800, 600, 90, gray=True))
    return datas


@pytest.fixture(scope="module")
def twelve():
    datas = _twelve()
    std = _files(_ctx(False, 92, **RESIZE), datas, "option off")
    want = []
    for s in std:
        tw = R.optimise(s)
        assert not tw.fallback and len(tw.file) < len(s)
        want.append(tw.file)
    return datas, want


def test_path_decode_batch(twelve):
    datas, want = twelve
    for i, (g, w) in enumerate(zip(_files(_ctx(True, 92, **RESIZE), datas), want)):
        _same(g, w, f"member {i}")


def test_path_torch(twelve):
    datas, want = twelve
    ctx = _ctx(True, 92, **RESIZE)
    for i, ((st, t, m), w) in enumerate(zip(ctx.decode_batch_torch(datas), want)):
        assert st == 0 and t.is_cuda and m.is_encoded == 1 and m.channels == -1 and m.nbytes == len(w), i
        _same(t.cpu().numpy().tobytes()[:m.nbytes], w, f"member {i}")


def test_path_submit_host(twelve):
    datas, want = twelve
    ctx = _ctx(True, 92, **RESIZE)
    caps = [ctx.output_size(d)[1] for d in datas]
    assert caps == [_ctx(False, 92, **RESIZE).output_size(d)[1] for d in datas]  # the bound does not move
    outs = [np.full(c, 0xA5, np.uint8) for c in caps]
    ticket, metas, keep = ctx.submit_host(datas, outs)
    ctx.wait(ticket)
    for i, (o, m, w) in enumerate(zip(outs, metas, want)):
        assert m.status == 0 and m.is_encoded == 1 and m.channels == -1 and m.nbytes == len(w), (i, _lib().last_error())
        _same(o[:m.nbytes].tobytes(), w, f"member {i}")
        assert (o[m.nbytes:] == 0xA5).all(), i
    del keep


def test_path_decode_one_coalesced(twelve):
    datas, want = twelve
    ctx = _ctx(True, 92, **RESIZE)
    ctx.set_option("coalesce_us", 20000)
    res = [None] * len(datas)

    def work(k):
        for i in range(k, len(datas), 8):
            res[i] = ctx.decode_one(datas[i])

    th = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for i, ((st, buf, m), w) in enumerate(zip(res, want)):
        assert st == 0 and m.is_encoded == 1 and m.nbytes == len(w), (i, _lib().last_error())
        _same(buf.tobytes()[:m.nbytes], w, f"member {i}")
    assert ctx.stat("coalesced_images") > 0


def test_path_budget_split(twelve):
    datas, want = twelve

    def fresh(optimize):
        c = _ctx(optimize, 92, **RESIZE)
        c.set_option("coef_cache_mb", 0)
        return c

    def exact_mb(items):  # footprint at exact sizes: no growth headroom, no prewarmed idle slots
        r = fresh(True)
        r.set_option("budget_plan", 0)
        r.set_option("max_device_mb", 1 << 20)
        assert all(st == 0 for st, _, _ in r.decode_batch(items)), _lib().last_error()
        mb = r.stat("peak_device_mb")
        r.close()
        return mb
    from datago_amd import synth
    base, peak = exact_mb([synth.make_jpeg(1, 32, 32, 90)]), exact_mb(datas)
    assert peak > base
    c = fresh(True)
    c.set_option("max_device_mb", base + max(8, (peak - base) // 3))
    got = _files(c, datas)
    assert c.stat("budget_splits") > 0, (peak, base)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"member {i}")
    c.close()


# ------------------------------------------------------------------ 5. surface

def test_transform_and_sample(twelve):
    from datago_amd import samples as S
    from datago_amd.image_processing import ARAwareTransform, ImageEncoding, ImageTransformConfig
    datas, want = twelve
    cfg = ImageTransformConfig(crop_and_resize=True, default_image_size=512, downsampling_ratio=32,
                               min_aspect_ratio=0.5, max_aspect_ratio=2.0)
    enc = ImageEncoding(encode_images=True, encode_format=FMT_JPEG, jpeg_quality=92)
    tfm = ARAwareTransform(cfg, 0, jenc_optimize=True)
    for i, (g, w) in enumerate(zip(_files(tfm.context(enc), datas[:4]), want[:4])):
        _same(g, w, f"member {i}")
    out = S.process_sample(S.TarballSample("s", [S.BinaryFile("a.jpg", datas[0])]), tfm, enc)
    assert out is not None and not out.unsupported and out.image.is_encoded and out.image.channels == -1
    _same(bytes(out.image.data), want[0], "the sample's image")
    off = S.process_sample(S.TarballSample("s", [S.BinaryFile("a.jpg", datas[0])]), ARAwareTransform(cfg, 0), enc)
    assert len(bytes(off.image.data)) > len(want[0]) and R.optimise(bytes(off.image.data)).file == want[0]

"""The option table (datago_amd/csrc/host/options.cpp) without a GPU: every
dg_ctx_set_option key's accepted and rejected values, the dg_last_error text of
a rejection and the defaults, through apply_option on a fresh Options
(tests/native/options_main.cpp, built with plain g++).  The expectations are
the checks of Context::set_option as it stood before the table."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EXE = os.path.join(NATIVE, "options_main")
HOST = os.path.join(ROOT, "datago_amd", "csrc", "host")


def build_options_main():
    srcs = [os.path.join(NATIVE, "options_main.cpp"), os.path.join(HOST, "options.cpp")]
    deps = srcs + [os.path.join(HOST, "options.h"), os.path.join(ROOT, "datago_amd", "csrc", "dg_types.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(p) > os.path.getmtime(EXE) for p in deps):
        tmp = f"{EXE}.{os.getpid()}.tmp"  # build beside it and rename: parallel workers never run half a file
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "datago_amd", "csrc"),
                        "-o", tmp] + srcs, check=True)
        os.replace(tmp, EXE)
    return EXE


def option_defaults():
    """{key: the value that leaves a fresh context's option as it is}, in table order."""
    out = subprocess.run([build_options_main(), "list"], check=True, capture_output=True, text=True).stdout
    rows = [ln.split("\t") for ln in out.splitlines()]
    return [r[0] for r in rows], {r[0]: int(r[1]) for r in rows if r[1] != "-"}


BIG = 1 << 40
W01 = "valid unless v < 0 || v > 1"


def flag(invert=False):  # the older flags: any value, stored as v != 0 (png_chunked: v == 0)
    on, off = (0, 1) if invert else (1, 0)
    return {"stored": {0: off, 1: on, 2: on, -1: on, BIG: on}, "rejected": {}}


def rng(lo, hi, why, scale=1, mid=()):  # lo <= v <= hi (hi None: no upper bound); the field holds v * scale
    stored = {v: v * scale for v in (lo, hi if hi is not None else BIG) + tuple(mid)}
    rejected = {lo - 1: why, -BIG: why}
    if hi is not None:
        rejected.update({hi + 1: why, BIG: why})
    return {"stored": stored, "rejected": rejected}


def strict():  # the newer flags: 0 and 1 only
    return {"stored": {0: 0, 1: 1}, "rejected": {-1: W01, 2: W01, BIG: W01}}


def pow2(lo, hi, why, zero=False, inside=()):  # powers of two in lo..hi (zero: and 0); inside: in range, no member
    stored = {v: v for v in (lo, 2 * lo, hi)}
    rejected = {v: why for v in (lo - 1, lo + 1, lo // 2, hi - 1, hi + 1, 2 * hi, -1, -lo, BIG) + tuple(inside)}
    if zero:
        stored[0] = 0
    else:
        rejected[0] = why
    return {"stored": stored, "rejected": rejected}


def raw(wrap):  # no check: the value cast to the field's type
    return {"stored": {0: 0, 1: 1, 7: 7, -1: wrap(-1), BIG + 5: wrap(BIG + 5)}, "rejected": {}}


def as_i32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def as_u32(v):
    return v % (1 << 32)


CASES = {
    "sub_bits": pow2(64, 65536, "valid unless v != 0 && (v < 64 || v > 65536 || (v & (v - 1)))", zero=True,
                     inside=(96, 100)),
    "sub_auto": pow2(1024, 65536, "valid unless v < 1024 || v > 65536 || (v & (v - 1))", inside=(3000,)),
    "lead_bits": rng(-1, 1 << 20, "valid unless v < -1 || v > (1 << 20)", mid=(0,)),
    "coalesce_max": rng(1, 4096, "valid unless v < 1 || v > 4096"),
    "coalesce_inflight": rng(0, 6, "valid unless v < 0 || v > 6"),
    "coalesce_us": rng(0, 1000000, "valid unless v < 0 || v > 1000000"),
    "wg_timing": flag(),
    "timing": flag(),
    "side_stream": flag(),
    "coef_cache_mb": rng(0, 65536, "valid unless v < 0 || v > 65536", scale=1 << 20, mid=(1,)),
    "entropy_prio": rng(0, 3, "valid unless v < 0 || v > 3"),
    "max_device_mb": rng(0, None, "valid unless v < 0", scale=1 << 20, mid=(1,)),
    "budget_plan": flag(),
    "slots": rng(1, 6, "valid unless v < 1 || v > 6"),
    "progressive": flag(),
    "png16": strict(),
    "gif": strict(),
    "webp": strict(),
    "jpeg_h1v2": strict(),
    "jpeg_cmyk": strict(),
    "jpeg_multiscan": strict(),
    "resize16": strict(),
    "penc16": strict(),
    "penc_dynamic": strict(),
    "jenc_optimize": strict(),
    "prog_lanes": rng(0, 2, "valid unless v < 0 || v > 2"),
    "prog_queue": rng(0, 3, "valid unless v < 0 || v > 3"),
    "slot_queue": rng(0, 3, "valid unless v < 0 || v > 3"),
    "side_queue": rng(-1, 3, "valid unless v < -1 || v > 3"),
    "prog_cus": rng(0, 4096, "valid unless v < 0 || v > 4096"),
    "prog_split": flag(),
    "prog_batch": rng(1, 65536, "valid unless v < 1 || v > 65536"),
    "prog_flush_us": rng(0, 100000000, "valid unless v < 0 || v > 100000000"),
    "sync2": flag(),
    "sync_pair": flag(),
    "sync_chain": rng(0, 3, "valid unless v < 0 || v > 3"),
    "write_pair": rng(0, 3, "valid unless v < 0 || v > 3"),
    "multi_lead": flag(),
    "prog_side": flag(),
    "prog_chain": rng(0, 100000, "valid unless v < 0 || v > 100000"),
    "prog_pipe": flag(),
    "prog_serial": flag(),
    "entropy_once": flag(),
    "entropy_lpt": flag(),
    "hb_bands": rng(1, 64, "valid unless v < 1 || v > 64"),
    "idct_fused": flag(),
    "idct_thread": flag(),
    "sparse_coef": flag(),
    "h_prefetch": flag(),
    "h_planar": flag(),
    "destuff_one": flag(),
    "chroma_rec": flag(),
    "reset_host_us": {"stored": {0: "-", 1: "-", -1: "-", BIG: "-"}, "rejected": {}},  # no field: a signal
    "hv_fused": flag(),
    "copy_threads": rng(1, 64, "valid unless v < 1 || v > 64"),
    "ckpt": flag(),
    "decode_semantics": rng(0, 1, "valid unless v != 0 && v != 1"),
    "small_coded": rng(0, None, "valid unless v < 0", mid=(1,)),
    "sub_small": pow2(64, 65536, "valid unless v < 64 || v > 65536 || (v & (v - 1))", inside=(96,)),
    "lead_small": rng(0, 1 << 16, "valid unless v < 0 || v > (1 << 16)"),
    "v_tile": {"stored": {0: 0, 2: 2, 4: 4, 8: 8},
               "rejected": {v: "valid: 0, 2, 4, 8" for v in (-1, 1, 3, 5, 6, 7, 9, 16, -2, -8, BIG)}},
    "v_units": rng(1, 8, "valid unless v < 1 || v > 8"),
    "lead_big": rng(0, 1 << 16, "valid unless v < 0 || v > (1 << 16)"),
    "write_split": flag(),
    "meta_pull": rng(0, 2, "valid unless v < 0 || v > 2"),
    "plan_threads": rng(1, 64, "valid unless v < 1 || v > 64"),
    "inf_stage3": {"stored": {8: 8, 16: 16, 32: 32, 64: 64},
                   "rejected": {v: "valid unless v != 8 && v != 16 && v != 32 && v != 64"
                                for v in (0, 1, 4, 7, 9, 24, 63, 65, 128, -8, BIG)}},
    "inf_cap": rng(10, 100, "valid unless v < 10 || v > 100"),
    "png_alias": flag(),
    "inf_pad": rng(0, 1 << 20, "valid unless v < 0 || v > 2^20"),
    "inf_chunk": pow2(4096, 65536, "valid unless v < 4096 || v > 65536 || (v & (v - 1))", inside=(5000,)),
    "png_chunked": flag(invert=True),  # stored into chunked_off
    "lead_density": flag(),
    "sub_density": rng(0, 4096, "valid unless v < 0 || v > 4096", mid=(7,)),
    "uf_per_cu": rng(0, 16, "valid unless v < 0 || v > 16"),
    "uf_units": rng(1, 2, "valid unless v < 1 || v > 2"),
    "inf_decode": {"stored": {0: 0, 9: 9, 11: 11, 28: 28},
                   "rejected": {v: "valid unless v < 0 || v > 28 || v == 10" for v in (-1, 10, 29, BIG, -BIG)}},
    "h_mfma": flag(),
    "band_dec": flag(),
    "dec_dbg": raw(as_u32),
    "dec_strips": rng(1, 4096, "valid unless v < 1 || v > 4096"),
    "debug_flags": raw(as_i32),
}

# the defaults of a fresh context, as option values
DEFAULTS = {
    "sub_bits": 0, "sub_auto": 8192, "lead_bits": -1, "coalesce_max": 64, "coalesce_inflight": 3, "coalesce_us": 500,
    "wg_timing": 0, "timing": 0, "side_stream": 1, "coef_cache_mb": 256, "entropy_prio": 0, "max_device_mb": 0,
    "budget_plan": 1, "slots": 4, "progressive": 1, "png16": 0, "gif": 0, "webp": 0, "jpeg_h1v2": 0, "jpeg_cmyk": 0,
    "jpeg_multiscan": 0, "resize16": 0, "penc16": 0, "penc_dynamic": 0, "jenc_optimize": 0, "prog_lanes": 1,
    "prog_queue": 2, "slot_queue": 1, "side_queue": 3, "prog_cus": 0, "prog_split": 1, "prog_batch": 2048,
    "prog_flush_us": 20000, "sync2": 0, "sync_pair": 0, "sync_chain": 2, "write_pair": 3, "multi_lead": 1,
    "prog_side": 0, "prog_chain": 100, "prog_pipe": 1, "prog_serial": 0, "entropy_once": 0, "entropy_lpt": 1,
    "hb_bands": 16, "idct_fused": 0, "idct_thread": 1, "sparse_coef": 1, "h_prefetch": 1, "h_planar": 1,
    "destuff_one": 0, "chroma_rec": 1, "hv_fused": 0, "copy_threads": 8, "ckpt": 1, "decode_semantics": 0,
    "small_coded": 0, "sub_small": 512, "lead_small": 1024, "v_tile": 4, "v_units": 2, "lead_big": 4096,
    "write_split": 1, "meta_pull": 1, "plan_threads": 4, "inf_stage3": 32, "inf_cap": 30, "png_alias": 1,
    "inf_pad": 65536, "inf_chunk": 32768, "png_chunked": 1, "lead_density": 0, "sub_density": 0, "uf_per_cu": 0,
    "uf_units": 1, "inf_decode": 25, "h_mfma": 0, "band_dec": 0, "dec_dbg": 0, "dec_strips": 8, "debug_flags": 0,
}


@pytest.fixture(scope="module")
def table():
    return option_defaults()


@pytest.fixture(scope="module")
def results():
    """Every (key, value) of CASES through apply_option on a fresh Options, in one run of the program:
    {(key, value): (status, field, unchanged, text)}."""
    queries = [(k, v) for k, c in CASES.items() for v in list(c["stored"]) + list(c["rejected"])]
    queries.append(("no_such_option", 1))
    args = [s for k, v in queries for s in (k, str(v))]
    out = subprocess.run([build_options_main(), "apply"] + args, check=True, capture_output=True, text=True).stdout
    lines = out.split("\n")[:-1]
    assert len(lines) == len(queries)
    res = {}
    for q, ln in zip(queries, lines):
        st, field, same, text = ln.split("\t")
        res[q] = (int(st), field, int(same), text)
    return res


def test_table_has_no_duplicates_and_every_key_has_cases(table):
    names, _ = table
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    assert set(names) == set(CASES), set(names) ^ set(CASES)


@pytest.mark.parametrize("key", list(CASES))
def test_option_takes_and_rejects_what_it_did(results, table, key):
    # the field at its default, where the cases hold that value: storing it again changes nothing, any other does
    dfield = CASES[key]["stored"].get(table[1].get(key))
    for v, want in CASES[key]["stored"].items():
        st, field, same, text = results[(key, v)]
        assert (st, field, text) == (0, str(want), ""), (key, v, results[(key, v)])
        if dfield is not None:
            assert same == (want == dfield), (key, v)
    for v, why in CASES[key]["rejected"].items():
        st, field, same, text = results[(key, v)]
        assert st == 1 and text == f'dg_ctx_set_option("{key}", {v}): {why}', (key, v, results[(key, v)])
        assert same == 1, (key, v)  # a rejected value leaves the Options byte for byte as they were


def test_unknown_option(results):
    assert results[("no_such_option", 1)] == (2, "-", 1, 'dg_ctx_set_option("no_such_option", 1): unknown option')


@pytest.mark.parametrize("key,v,text", [
    ("slots", 0, 'dg_ctx_set_option("slots", 0): valid unless v < 1 || v > 6'),
    ("prog_lanes", 3, 'dg_ctx_set_option("prog_lanes", 3): valid unless v < 0 || v > 2'),
    ("v_tile", 3, 'dg_ctx_set_option("v_tile", 3): valid: 0, 2, 4, 8'),
    ("inf_decode", 10, 'dg_ctx_set_option("inf_decode", 10): valid unless v < 0 || v > 28 || v == 10'),
    ("webp", 2, 'dg_ctx_set_option("webp", 2): valid unless v < 0 || v > 1'),
    ("decode_semantics", 2, 'dg_ctx_set_option("decode_semantics", 2): valid unless v != 0 && v != 1'),
    ("inf_pad", 1048577, 'dg_ctx_set_option("inf_pad", 1048577): valid unless v < 0 || v > 2^20'),
    ("sub_bits", 100,
     'dg_ctx_set_option("sub_bits", 100): valid unless v != 0 && (v < 64 || v > 65536 || (v & (v - 1)))'),
    ("no_such_option", 1, 'dg_ctx_set_option("no_such_option", 1): unknown option'),
])
def test_rejection_texts_in_full(results, key, v, text):
    st, field, same, got = results[(key, v)]
    assert st != 0 and same == 1 and got == text


def test_defaults(table):
    _, defaults = table
    assert defaults == DEFAULTS
    # the ones with history (each was measured into its value)
    for key, v in [("slots", 4), ("write_pair", 3), ("sync_chain", 2), ("inf_decode", 25), ("v_tile", 4),
                   ("coalesce_inflight", 3), ("prog_batch", 2048), ("inf_cap", 30), ("inf_pad", 65536),
                   ("progressive", 1)]:
        assert defaults[key] == v, key
    for key in ("png16", "gif", "webp", "jpeg_h1v2", "jpeg_cmyk", "jpeg_multiscan", "resize16", "penc16",
                "penc_dynamic", "jenc_optimize"):
        assert defaults[key] == 0, key

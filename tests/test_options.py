"""pl_options (include/libplacebo/options.h): the option-string front end of pl_render_params.

* the header is layout-identical to the reference's: tests/golden/abi_layout_options.json
  (`tools/abi_probe.py golden-options`, from the reference's header), the same mechanism as
  tests/test_abi_layout.py, with the ctypes mirrors (_capi.MIRRORS_OPTIONS) held to the same table;
* the option list is the reference's, entry for entry: tests/golden/options_list.json holds
  (key, type, min, max, deprecated, preset) and the value names of every enum and preset list, as
  printed from the reference's option table by a throw-away program;
* the scenario of the reference's own src/tests/options.c, with the expected strings derived from
  this library's preset structs;
* every option survives save -> reset -> load byte for byte, every preset value loads, every
  malformed entry is refused with one error and without a change.
No GPU needed."""
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np
import pytest

import libplacebo_amd as pl
from libplacebo_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_probe  # noqa: E402

GOLDEN = abi_probe.GROUPS["options"][1]
HAVE_REF = os.path.isdir(os.path.join(abi_probe.REF, "src", "include")) and \
    os.path.exists(os.path.join(ROOT, "oracle", "_ref", "gen", "libplacebo", "config.h"))
AGGREGATES = ["struct pl_options_t", "struct pl_opt_t", "struct pl_opt_data_t"]
LIST = json.load(open(os.path.join(ROOT, "tests", "golden", "options_list.json")))
BY_KEY = {e["key"]: e for e in LIST}

STRUCTS = ["deband_params", "sigmoid_params", "color_adjustment", "peak_detect_params",
           "color_map_params", "dither_params", "icc_params", "cone_params", "blend_params",
           "deinterlace_params", "distort_params"]
SCALERS = {"upscaler": pl.FILTER_UPSCALING, "downscaler": pl.FILTER_DOWNSCALING,
           "plane_upscaler": pl.FILTER_UPSCALING, "plane_downscaler": pl.FILTER_DOWNSCALING,
           "frame_mixer": pl.FILTER_FRAME_MIXING}
# the tables of named objects the library exports, by the option that takes one of them
NAMED = {"gamut_mapping": "pl_gamut_map_functions", "tone_mapping": "pl_tone_map_functions",
         "error_diffusion": "pl_error_diffusion_kernels"}
NAMED.update({f"{s}_{part}": "pl_filter_functions" for s in SCALERS for part in ("kernel", "window")})
# the struct behind each per-struct preset value (cone presets: pl_vision_<value>)
PRESET_SYMBOL = {
    "deband_preset": "pl_deband_{}_params", "sigmoid_preset": "pl_sigmoid_{}_params",
    "color_adjustment_preset": "pl_color_adjustment_{}", "peak_detect_preset": "pl_peak_detect_{}_params",
    "color_map_preset": "pl_color_map_{}_params", "dither_preset": "pl_dither_{}_params",
    "icc_preset": "pl_icc_{}_params", "cone_preset": "pl_vision_{}", "blend_preset": "pl_{}",
    "deinterlace_preset": "pl_deinterlace_{}_params", "distort_preset": "pl_distort_{}_params"}


def norm(table):
    return {k: (tuple(v) if isinstance(v, list) else v) for k, v in table.items()}


class Log:
    """a pl_log that keeps its messages"""

    def __init__(self):
        self.msgs = []
        self._cb = capi.LOG_CB(lambda _p, lev, msg: self.msgs.append((lev, msg.decode())))
        lp = capi.LogParams(log_cb=self._cb, log_priv=None, log_level=3)
        self.log = C.c_void_p(pl.lib().pl_log_create_365(365, C.byref(lp)))

    def errors(self):
        return [m for lev, m in self.msgs if lev <= 2]

    def close(self):
        pl.lib().pl_log_destroy(C.byref(self.log))


@pytest.fixture()
def opts(built):
    """a fresh pl_options with a log that keeps its messages; its pointers are checked on the way out"""
    log = Log()
    o = pl.Options(log.log)
    o.log = log
    yield o
    check_pointers(o)
    o.free()
    assert not o.ptr
    log.close()


def table_names(symbol):
    """names of a NULL-terminated array of pointers to structs that begin with their name"""
    n = C.c_int.in_dll(pl.lib(), symbol.replace("pl_", "pl_num_", 1)).value
    arr = (C.POINTER(C.c_char_p) * n).in_dll(pl.lib(), symbol)
    return [arr[i].contents.value.decode() for i in range(n)]


def filter_configs(usage):
    """[(name, address)] of the built-in filter configs allowed for `usage`"""
    n = C.c_int.in_dll(pl.lib(), "pl_num_filter_configs").value
    arr = (C.POINTER(capi.FilterConfig) * n).in_dll(pl.lib(), "pl_filter_configs")
    return [(arr[i].contents.name.decode(), C.addressof(arr[i].contents)) for i in range(n)
            if arr[i].contents.allowed & usage]


def address(ptr):
    return C.cast(ptr, C.c_void_p).value


def check_pointers(o):
    """every non-NULL params.*_params points at the member of the same name of the same object;
    every scaler at a built-in config or at its own slot"""
    base = C.addressof(o.struct)
    for f in STRUCTS:
        p = address(getattr(o.params, f))
        assert p in (None, base + getattr(capi.Options, f).offset), f
    builtin = {a for _, a in filter_configs(7)}
    for f in SCALERS:
        p = address(getattr(o.params, f))
        assert p is None or p == base + getattr(capi.Options, f).offset or p in builtin, f
        slot = getattr(o.struct, f)
        assert slot.name == b"custom" and slot.description and slot.allowed == SCALERS[f], f


# ---- layout -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ours():
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    return norm(abi_probe.run_probe("ours", abi_probe.aggregates("ours", "options"), group="options"))


@pytest.fixture(scope="module")
def golden():
    return norm(json.load(open(GOLDEN)))


def test_every_member_has_the_references_offset_and_size(ours, golden):
    assert {k for k in golden if "." not in k} == set(AGGREGATES)
    assert len([k for k in golden if k.startswith("struct pl_options_t.")]) == 1 + 11 + 5
    bad = {k: (ours.get(k), v) for k, v in golden.items() if ours.get(k) != v}
    assert not bad, bad
    assert set(ours) == set(golden), sorted(set(ours) ^ set(golden))


@pytest.mark.skipif(not HAVE_REF, reason="reference headers not present")
def test_golden_is_what_the_reference_header_gives(golden):
    live = norm(abi_probe.run_probe("ref", group="options"))
    assert live == golden, "abi_layout_options.json is stale: run tools/abi_probe.py golden-options"


def test_ctypes_mirrors_match_the_header(ours):
    assert set(capi.MIRRORS_OPTIONS) == set(AGGREGATES)
    bad = []
    for cname, mirror in capi.MIRRORS_OPTIONS.items():
        if C.sizeof(mirror) != ours[cname]:
            bad.append((cname, "sizeof", C.sizeof(mirror), ours[cname]))
        for fname, *_ in mirror._fields_:
            key = f"{cname}.{fname}"
            assert key in ours, key
            f = getattr(mirror, fname)
            if (f.offset, f.size) != ours[key]:
                bad.append((key, (f.offset, f.size), ours[key]))
        n_c = sum(1 for k in ours if k.startswith(cname + "."))
        if n_c != len(mirror._fields_):
            bad.append((cname, "member count", len(mirror._fields_), n_c))
    assert not bad, bad
    assert C.sizeof(capi.IccParams) == ours["struct pl_options_t.icc_params"][1]


# ---- the list -------------------------------------------------------------------------------------

def test_option_list_is_the_references(built):
    got = pl.option_list()
    assert C.c_int.in_dll(pl.lib(), "pl_option_count").value == len(LIST) == len(got)
    for o, e in zip(got, LIST):
        assert (o.key.decode(), o.type, o.min, o.max, o.deprecated, o.preset) == \
            (e["key"], e["type"], np.float32(e["min"]), np.float32(e["max"]), e["deprecated"],
             e["preset"]), e["key"]
        assert o.name and o.priv
    end = (capi.Opt * (len(LIST) + 1)).in_dll(pl.lib(), "pl_option_list")[len(LIST)]
    assert not end.key and not end.name and not end.priv    # the {0} that ends the list
    assert len(BY_KEY) == len(LIST)


def test_find_option(built):
    L = pl.lib()
    base = C.addressof((capi.Opt * len(LIST)).in_dll(L, "pl_option_list"))
    for i, e in enumerate(LIST):
        found = L.pl_find_option(e["key"].encode())
        assert found and C.addressof(found.contents) == base + i * C.sizeof(capi.Opt), e["key"]
    for key in (b"", b"bogus", b"Preset", b"upscaler_"):
        assert not L.pl_find_option(key)


# ---- the reference's scenario -----------------------------------------------------------------------

def shortest(x):
    """a float32 as options print it: the shortest text that reads back as the same value"""
    return repr(float(np.float32(x))).removesuffix(".0")


def expected_save(preset):
    """what a preset struct of this library saves as (the members its presets use)"""
    p = capi.RenderParams.in_dll(pl.lib(), f"pl_render_{preset}_params")
    out = [f"{f}={getattr(p, f).contents.name.decode()}" for f in ("upscaler", "downscaler", "frame_mixer")
           if getattr(p, f)]
    if p.deband_params:
        out.append("deband=yes")
    if p.sigmoid_params:
        out.append("sigmoid=yes")
    if p.peak_detect_params:
        out.append("peak_detect=yes")
        percentile = p.peak_detect_params.contents.percentile
        if percentile != capi.PeakDetectParams.in_dll(pl.lib(), "pl_peak_detect_default_params").percentile:
            out.append(f"peak_percentile={shortest(percentile)}")
    recovery = p.color_map_params.contents.contrast_recovery
    if recovery:
        out.append(f"contrast_recovery={shortest(recovery)}")
    if p.dither_params:
        out.append("dither=yes")
    return ",".join(out)


def test_fresh_object_is_the_fast_preset(opts):
    assert opts.save() == ""
    assert opts.load("") and opts.save() == ""
    fresh = opts.raw()
    opts.reset("fast")
    assert opts.save() == "" and opts.raw() == fresh
    assert opts.load("preset=fast") and opts.save() == "" and opts.raw() == fresh
    assert opts.iterate() == []
    # the empty configuration is pl_render_fast_params with its two structs taken inside
    fast = capi.RenderParams.in_dll(pl.lib(), "pl_render_fast_params")
    assert opts.params.tile_size == fast.tile_size == 32 and not opts.params.upscaler
    assert opts.params.color_map_params and opts.params.color_adjustment
    assert not opts.log.msgs


@pytest.mark.parametrize("preset", ["default", "high_quality"])
def test_presets_round_trip(opts, preset):
    want = expected_save(preset)
    opts.reset(preset)
    saved = opts.save()
    if preset == "high_quality" and "658203125" in saved:       # (the longer spelling of 99.995f)
        want = want.replace("99.99500274658203", "99.99500274658203125")
    assert saved == want
    after_reset = opts.raw()
    assert len(opts.iterate()) == len(want.split(","))
    assert [f"{k}={v}" for k, v in opts.iterate()] == want.split(",")

    opts.reset(None)
    assert opts.save() == ""
    assert opts.load(want) and opts.save() == want
    assert opts.raw() == after_reset
    opts.reset(None)
    assert opts.load(f"preset={preset}") and opts.save() == want
    assert opts.raw() == after_reset

    value, text = opts.get("tile_size")
    assert text == "32"
    assert C.c_int.from_address(value).value == 32 == \
        capi.RenderParams.in_dll(pl.lib(), f"pl_render_{preset}_params").tile_size
    assert value == C.addressof(opts.struct) + capi.RenderParams.tile_size.offset
    assert not opts.log.errors()


def test_preset_strings(opts):
    assert expected_save("default") == \
        "upscaler=lanczos,downscaler=hermite,sigmoid=yes,peak_detect=yes,dither=yes"
    hq = expected_save("high_quality")
    assert "peak_percentile=99.99500274658203," in hq
    assert "contrast_recovery=0.30000001192092896," in hq
    opts.reset("high_quality")
    assert opts.get("peak_percentile")[1] in ("99.99500274658203", "99.99500274658203125")
    assert opts.get("contrast_recovery")[1] == "0.30000001192092896"


def test_iterating_into_another_object_copies_the_configuration(opts):
    opts.reset("high_quality")
    other = pl.Options()
    for key, text in opts.iterate():
        assert other.set(key, text)
    assert other.save() == opts.save()
    check_pointers(other)
    other.free()


def test_custom_scaler(opts):
    """a scaler that is no built-in config is copied into its slot; the same configuration can be
    spelt as a preset plus two overrides"""
    L = pl.lib()
    jinc = C.pointer(capi.FilterFunction.in_dll(L, "pl_filter_function_jinc"))
    cfg = capi.FilterConfig(kernel=jinc, window=jinc, radius=4.0, polar=True)
    opts.reset(pl.render_params("fast", upscaler=cfg))
    want = "upscaler=custom,upscaler_kernel=jinc,upscaler_window=jinc,upscaler_radius=4,upscaler_polar=yes"
    assert opts.save() == want
    assert address(opts.params.upscaler) == C.addressof(opts.struct) + capi.Options.upscaler.offset
    before = opts.raw()
    opts.reset(None)
    assert opts.load("upscaler=custom,upscaler_preset=ewa_lanczos,upscaler_radius=4.0,upscaler_clamp=0.0")
    assert opts.save() == want and opts.raw() == before
    # resetting an object from its own params keeps what they point to
    opts.reset(opts.params)
    assert opts.save() == want and opts.raw() == before


def test_reset_from_a_custom_scaler_keeps_all_of_it(opts):
    """antiring and the parameters included; the slot keeps its own name, description and usages"""
    hann = C.pointer(capi.FilterFunction.in_dll(pl.lib(), "pl_filter_function_hann"))
    cfg = capi.FilterConfig(name=b"mine", description=b"my filter", allowed=7, recommended=7,
                            kernel=hann, radius=2.5, params=(C.c_float * 2)(0.25, 0.5),
                            wparams=(C.c_float * 2)(1.5, 2.0), clamp=0.125, blur=1.25, taper=0.0625,
                            antiring=0.75)
    opts.reset(pl.render_params("fast", downscaler=cfg))
    want = ("downscaler=custom,downscaler_kernel=hann,downscaler_radius=2.5,downscaler_clamp=0.125,"
            "downscaler_blur=1.25,downscaler_taper=0.0625,downscaler_antiring=0.75,"
            "downscaler_param1=0.25,downscaler_param2=0.5,downscaler_wparam1=1.5,downscaler_wparam2=2")
    assert opts.save() == want
    slot = opts.struct.downscaler
    assert (slot.name, slot.allowed, slot.recommended) == (b"custom", pl.FILTER_DOWNSCALING, 0)
    before = opts.raw()
    opts.reset(opts.params)
    assert opts.save() == want and opts.raw() == before
    opts.reset(None)
    assert opts.load(want) and opts.raw() == before


def test_committed_table_is_what_the_generator_writes():
    """csrc/host/options_table.inc comes from tests/golden/options_list.json through
    tools/gen_options_table.py"""
    import gen_options_table
    assert open(gen_options_table.OUT).read() == gen_options_table.generate(), \
        "options_table.inc is stale: run tools/gen_options_table.py"


# ---- every option, there and back ---------------------------------------------------------------------

def candidates(e):
    """legal texts for a non-preset option: the second name of a list, both ends of a range, a
    value inside it and a fraction"""
    key, lo, hi = e["key"], e["min"], e["max"]
    if e["type"] == capi.OPT_BOOL:
        return ["yes", "no", "on", "off", "true", "false", "y", "n", "enabled", "disabled"]
    if e["type"] == capi.OPT_INT:
        return [str(int(lo)), str(int(hi)), str(int(lo + hi) // 2)] if lo != hi else ["-3", "7", "+12"]
    if e["type"] == capi.OPT_FLOAT:
        if lo == hi:
            return ["-2.5", "0.37", "1e-3", "1/3", "-7/3", "3"]
        frac = next(f for f, v in (("1/3", 1 / 3), ("2/3", 2 / 3), ("7/3", 7 / 3)) if lo <= v <= hi)
        return [shortest(lo), shortest(hi), shortest((lo + hi) / 2), frac]
    if e["values"]:
        return e["values"]
    if key in NAMED:
        return ["none"] + table_names(NAMED[key])
    return ["none", "custom"] + [n for n, _ in filter_configs(SCALERS[key])]


@pytest.mark.parametrize("key", [e["key"] for e in LIST if not e["preset"]])
def test_round_trip(opts, key):
    e = BY_KEY[key]
    empty = opts.raw()
    texts = candidates(e)
    assert len(texts) >= 2
    default = opts.get(key)[1]
    changed = 0
    for text in texts:
        opts.reset(None)
        assert opts.set(key, text), (text, opts.log.msgs)
        value, printed = opts.get(key)
        assert C.addressof(opts.struct) <= value < C.addressof(opts.struct) + C.sizeof(capi.Options)
        if e["type"] == capi.OPT_INT:
            assert C.c_int.from_address(value).value == int(text) and printed == str(int(text))
        elif e["type"] == capi.OPT_FLOAT:
            num, _, den = text.partition("/")
            want = np.float32(num) / np.float32(den) if den else np.float32(text)
            assert C.c_float.from_address(value).value == want and printed == shortest(want)
        elif e["type"] == capi.OPT_STRING:
            assert printed == text
        else:
            assert printed == ("yes" if text in ("yes", "on", "true", "y", "enabled") else "no")

        saved, after = opts.save(), opts.raw()
        assert (saved == "") == (after == empty)
        assert saved == (f"{key}={printed}" if after != empty else "")
        assert opts.iterate() == ([(key, printed)] if saved else [])
        assert (after != empty) == (printed != default)
        changed += after != empty
        opts.reset(None)
        assert opts.raw() == empty
        assert opts.load(saved) and opts.raw() == after, saved
    assert changed >= 1
    assert not opts.log.errors()
    assert all("deprecated" in m for _, m in opts.log.msgs) and bool(opts.log.msgs) == e["deprecated"]


def test_everything_at_once(opts):
    """all non-default values in one object, through one string"""
    for e in LIST:
        if not e["preset"]:
            texts = candidates(e)
            default = opts.get(e["key"])[1]
            assert opts.set(e["key"], next(t for t in texts[1:] + texts[:1] if t != default))
    saved, after = opts.save(), opts.raw()
    assert [kv.split("=")[0] for kv in saved.split(",")] == [e["key"] for e in LIST if not e["preset"]]
    assert len(opts.iterate()) == len(LIST) - sum(e["preset"] for e in LIST)
    assert "hook" not in saved
    for sep in (",", ";", ":", " ", "\n", " ,\n; "):
        opts.reset(None)
        assert opts.load(saved.replace(",", sep)) and opts.raw() == after, repr(sep)
    opts.reset(None)
    assert opts.load(" \t" + saved.replace("=", "\t=\t").replace(",", "\t,\t") + ",,") and opts.raw() == after
    assert not opts.log.errors()


@pytest.mark.parametrize("key", [e["key"] for e in LIST if e["preset"]])
def test_presets_load_and_save_as_what_they_imply(opts, key):
    e = BY_KEY[key]
    slot = key[:-len("_preset")]
    values = e["values"] or ["none"] + [n for n, _ in filter_configs(SCALERS[slot])]
    assert opts.get(key) is None and len(opts.log.errors()) == 1
    del opts.log.msgs[:]
    for value in values:
        opts.reset(None)
        assert opts.load(f"{key}={value}"), (value, opts.log.msgs)
        saved, after = opts.save(), opts.raw()
        assert key + "=" not in saved
        if key == "preset":
            assert saved == expected_save(value)
        elif key in PRESET_SYMBOL:
            field = slot if slot in STRUCTS else slot + "_params"
            mirror = dict(capi.Options._fields_)[field]
            src = mirror.in_dll(pl.lib(), PRESET_SYMBOL[key].format(value))
            assert bytes(getattr(opts.struct, field)) == bytes(src), value
        else:
            got = getattr(opts.struct, slot)
            if value == "none":
                assert saved == ""
            else:
                cfg = pl.lib().pl_find_filter_config(value.encode(), SCALERS[slot]).contents
                assert cfg.name.decode() == value
                for f in ("radius", "clamp", "blur", "taper", "polar"):
                    assert getattr(got, f) == getattr(cfg, f), (value, f)
                assert address(got.kernel) == address(cfg.kernel)
                assert address(got.window) == address(cfg.window)
                assert list(got.params) == list(cfg.params) and list(got.wparams) == list(cfg.wparams)
                assert f"{slot}_kernel={cfg.kernel.contents.name.decode()}" in saved.split(",")
            assert not getattr(opts.params, slot)      # (filling the slot does not select it)
        opts.reset(None)
        assert opts.load(saved) and opts.raw() == after and opts.save() == saved
    assert not opts.log.errors()


def test_cone_preset_is_saved_as_its_values(opts):
    assert opts.load("cone=yes,cone_preset=deuteranomaly")
    assert opts.save() == "cone=yes,cones=m,cone_strength=0.5"


# ---- refusals -----------------------------------------------------------------------------------------

REFUSED = {
    "unknown key": "bogus=1", "int above its range": "deband_iterations=100",
    "int below its range": "lut_entries=-1", "float above its range": "brightness=2.0",
    "float below its range": "sigmoid_slope=0.5", "nan": "gamma=nan", "inf": "gamma=inf",
    "minus inf": "hue=-inf", "division by zero": "hue=1/0", "subnormal": "hue=1e-40",
    "float overflow": "hue=1e60", "unknown enum name": "dither_method=invalid",
    "unknown function": "tone_mapping=nope", "unknown filter": "upscaler=nope",
    "downscaler as upscaler preset": "frame_mixer=ewa_lanczos", "unknown preset": "preset=slow",
    "unknown scaler preset": "upscaler_preset=help", "not an int": "tone_lut_size=abc",
    "int with a tail": "tile_size=32x", "float as int": "tile_size=32.0",
    "not a boolean": "show_clipping=hello", "not a float": "gamma=oops",
    "hex float": "gamma=0x1p0", "half a fraction": "gamma=1/", "bare key of a number": "tile_size",
    "no key": "=", "two equals signs": "preset==bar", "bare word": "invalid",
    "exponent only": "peak_percentile=E8203125", "empty toggle value is fine but junk is not": "deband=maybe",
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_with_one_error_and_no_change(opts, case):
    assert opts.load("deband=yes,gamma=1.5,upscaler=custom,upscaler_preset=mitchell")
    before, saved = opts.raw(), opts.save()
    del opts.log.msgs[:]
    assert opts.load(REFUSED[case]) is False
    assert len(opts.log.errors()) == 1, opts.log.msgs
    key, _, value = REFUSED[case].partition("=")
    del opts.log.msgs[:]
    assert opts.set(key, value) is False
    assert len(opts.log.errors()) == 1, opts.log.msgs
    assert opts.raw() == before and opts.save() == saved


def test_get_refuses_presets_and_unknown_keys(opts):
    before = opts.raw()
    for key in ("preset", "deband_preset", "upscaler_preset", "bogus", ""):
        del opts.log.msgs[:]
        assert opts.get(key) is None
        assert len(opts.log.errors()) == 1, (key, opts.log.msgs)
    assert opts.raw() == before


def test_entries_after_a_bad_one_are_applied(opts):
    assert opts.load("deband=yes,bogus=1,dither=no") is False
    assert len(opts.log.errors()) == 1
    assert opts.params.deband_params and not opts.params.dither_params
    assert opts.save() == "deband=yes"
    opts.reset("default")
    assert opts.load("deband,bogus=1,dither=no") is False
    assert opts.params.deband_params and not opts.params.dither_params


def test_no_log_no_crash(built):
    o = pl.Options()
    assert not o.load("bogus=1") and o.get("bogus") is None and o.save() == ""
    o.free()
    o.free()
    pl.lib().pl_options_free(None)


# ---- pointers -------------------------------------------------------------------------------------

def test_toggling_keeps_the_values(opts):
    assert opts.load("deband=yes,deband_iterations=3,deband_grain=1.25")
    stored = bytes(opts.struct.deband_params)
    assert opts.load("deband=no") and not opts.params.deband_params
    assert bytes(opts.struct.deband_params) == stored
    assert opts.save() == "deband_iterations=3,deband_grain=1.25"
    assert opts.load("deband=yes")
    assert address(opts.params.deband_params) == C.addressof(opts.struct) + capi.Options.deband_params.offset
    assert opts.params.deband_params.contents.iterations == 3
    assert bytes(opts.struct.deband_params) == stored
    assert opts.save() == "deband=yes,deband_iterations=3,deband_grain=1.25"


def test_pointers_stay_inside_through_a_sequence(opts):
    toggles = ["deband", "sigmoid", "color_adjustment", "peak_detect", "color_map", "dither", "icc",
               "cone", "blend", "deinterlace", "distort"]
    for step in (lambda: opts.load(",".join(t + "=yes" for t in toggles)),
                 lambda: opts.load("preset=high_quality"),
                 lambda: opts.reset("default"),
                 lambda: opts.load("upscaler=custom,downscaler=custom,frame_mixer=custom,plane_upscaler=none"),
                 lambda: opts.reset(opts.params),
                 lambda: opts.load(",".join(t + "=no" for t in toggles)),
                 lambda: opts.load("preset=default,blend=yes,blend_preset=alpha_overlay"),
                 lambda: opts.reset(None)):
        step()
        check_pointers(opts)
    for t, f in zip(toggles, STRUCTS):
        assert opts.set(t, "yes")
        assert address(getattr(opts.params, f)) == C.addressof(opts.struct) + getattr(capi.Options, f).offset
    # the global preset keeps what no option reaches
    marker = capi.CustomLut()
    opts.params.lut = C.pointer(marker)
    opts.params.info_priv = 1234
    assert opts.load("preset=high_quality")
    assert address(opts.params.lut) == C.addressof(marker) and opts.params.info_priv == 1234
    opts.params.lut = None


# ---- hooks ------------------------------------------------------------------------------------------

def hook_list(o):
    arr = C.cast(o.params.hooks, C.POINTER(C.c_void_p))
    return [arr[i] for i in range(o.params.num_hooks)]


def test_hook_helpers(opts):
    h = [capi.Hook(signature=i) for i in range(6)]
    a = [C.addressof(x) for x in h]
    opts.add_hook(h[0])
    opts.add_hook(h[1])
    assert hook_list(opts) == [a[0], a[1]]
    opts.insert_hook(h[2], 0)
    assert hook_list(opts) == [a[2], a[0], a[1]]
    opts.insert_hook(h[3], -1)
    assert hook_list(opts) == [a[2], a[0], a[1], a[3]]
    opts.insert_hook(h[4], -2)
    assert hook_list(opts) == [a[2], a[0], a[1], a[4], a[3]]
    opts.insert_hook(h[5], 2)
    assert hook_list(opts) == [a[2], a[0], a[5], a[1], a[4], a[3]]
    opts.remove_hook_at(-1)
    assert hook_list(opts) == [a[2], a[0], a[5], a[1], a[4]]
    opts.remove_hook_at(0)
    opts.remove_hook_at(1)
    assert hook_list(opts) == [a[0], a[1], a[4]]
    assert opts.save() == "" and opts.iterate() == []
    # a preset loaded by name keeps them, a reset drops them
    assert opts.load("preset=default") and hook_list(opts) == [a[0], a[1], a[4]]
    assert "hook" not in opts.save()
    opts.reset("default")
    assert opts.params.num_hooks == 0 and not opts.params.hooks
    # an array of the caller's is copied, not written to
    mine = (C.c_void_p * 2)(a[3], a[4])
    opts.params.hooks, opts.params.num_hooks = C.cast(mine, C.c_void_p), 2
    opts.add_hook(h[5])
    assert hook_list(opts) == [a[3], a[4], a[5]] and list(mine) == [a[3], a[4]]
    assert opts.params.hooks != C.addressof(mine)
    for _ in range(3):
        opts.remove_hook_at(-1)
    assert opts.params.num_hooks == 0
    assert not opts.log.errors()
    opts.remove_hook_at(0)      # nothing there: one error, no change
    opts.insert_hook(h[0], 5)
    assert len(opts.log.errors()) == 2 and opts.params.num_hooks == 0

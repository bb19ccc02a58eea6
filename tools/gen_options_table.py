#!/usr/bin/env python3
"""Writes libplacebo_amd/csrc/host/options_table.inc, the rows of pl_option_list.

What an option is called, its type, range, flags, position and value names are API and come from
tests/golden/options_list.json. Where its value lives comes from this library's headers and is
stated here: per struct of pl_options_t, which member each key stands for (a member the key names
outright is not listed), and for every enum which constant each value name means. The human-readable
names are composed from the struct's label and the member.

    tools/gen_options_table.py            # rewrite the table
    tools/gen_options_table.py --print    # ... to stdout (tests/test_options.py compares)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = os.path.join(ROOT, "tests", "golden", "options_list.json")
OUT = os.path.join(ROOT, "libplacebo_amd", "csrc", "host", "options_table.inc")

SCALERS = {  # slot -> (label, usage)
    "upscaler": ("Upscaling filter", "PL_FILTER_UPSCALING"),
    "downscaler": ("Downscaling filter", "PL_FILTER_DOWNSCALING"),
    "plane_upscaler": ("Chroma upscaling filter", "PL_FILTER_UPSCALING"),
    "plane_downscaler": ("Chroma downscaling filter", "PL_FILTER_DOWNSCALING"),
    "frame_mixer": ("Frame mixing filter", "PL_FILTER_FRAME_MIXING"),
}
# key suffix -> member of struct pl_filter_config
SCALER_PARTS = {"kernel": "kernel", "window": "window", "radius": "radius", "clamp": "clamp",
                "blur": "blur", "taper": "taper", "antiring": "antiring", "param1": "params[0]",
                "param2": "params[1]", "wparam1": "wparams[0]", "wparam2": "wparams[1]",
                "polar": "polar"}

# member of pl_options_t -> (label, key that switches it on, prefix its keys carry, {key: member}
# for the keys that are not prefix + member)
STRUCTS = {
    "deband_params": ("Debanding", "deband", "deband_", {
        "deband_grain_neutral_r": "grain_neutral[0]", "deband_grain_neutral_g": "grain_neutral[1]",
        "deband_grain_neutral_b": "grain_neutral[2]"}),
    "sigmoid_params": ("Sigmoid", "sigmoid", "sigmoid_", {}),
    "color_adjustment": ("Colour adjustment", "color_adjustment", "", {}),
    "peak_detect_params": ("Peak measurement", "peak_detect", "", {
        "peak_smoothing_period": "smoothing_period", "peak_percentile": "percentile",
        "allow_delayed_peak": "allow_delayed"}),
    "color_map_params": ("Colour map", "color_map", "", {
        "lut3d_size_I": "lut3d_size[0]", "lut3d_size_C": "lut3d_size[1]", "lut3d_size_h": "lut3d_size[2]",
        "tone_mapping": "tone_mapping_function", "tone_map_metadata": "metadata",
        "tone_lut_size": "lut_size", "visualize_lut_x0": "visualize_rect.x0",
        "visualize_lut_y0": "visualize_rect.y0", "visualize_lut_x1": "visualize_rect.x1",
        "visualize_lut_y1": "visualize_rect.y1",
        **{k: "gamut_constants." + k for k in (
            "perceptual_deadzone", "perceptual_strength", "colorimetric_gamma", "softclip_knee",
            "softclip_desat")},
        **{k: "tone_constants." + k for k in (
            "knee_adaptation", "knee_minimum", "knee_maximum", "knee_default", "knee_offset",
            "slope_tuning", "slope_offset", "spline_contrast", "reinhard_contrast", "linear_knee",
            "exposure")}}),
    "dither_params": ("Dithering", "dither", "dither_", {}),
    "icc_params": ("ICC", "icc", "icc_", {}),
    "cone_params": ("Cone model", "cone", "cone_", {"cones": "cones"}),
    "blend_params": ("Blending", "blend", "blend_", {}),
    "deinterlace_params": ("Deinterlacing", "deinterlace", "deinterlace_", {
        "deinterlace_skip_spatial": "skip_spatial_check"}),
    "distort_params": ("Distortion", "distort", "distort_", {
        "distort_scale_x": "transform.mat.m[0][0]", "distort_scale_y": "transform.mat.m[1][1]",
        "distort_shear_x": "transform.mat.m[0][1]", "distort_shear_y": "transform.mat.m[1][0]",
        "distort_offset_x": "transform.c[0]", "distort_offset_y": "transform.c[1]"}),
}
# which struct the keys without a telling prefix belong to
MEMBERS_OF = {
    "color_adjustment": ("brightness", "contrast", "saturation", "hue", "gamma", "temperature"),
    "peak_detect_params": ("peak_smoothing_period", "scene_threshold_low", "scene_threshold_high",
                           "minimum_peak", "peak_percentile", "black_cutoff", "allow_delayed_peak"),
    "color_map_params": (
        "gamut_mapping", "lut3d_tricubic", "gamut_expansion", "inverse_tone_mapping",
        "contrast_recovery", "contrast_smoothness", "force_tone_mapping_lut", "visualize_lut",
        "visualize_hue", "visualize_theta", "show_clipping", "tone_mapping_param",
        *STRUCTS["color_map_params"][3]),
    "cone_params": ("cones",),
}
# keys of pl_render_params itself that are not the member's name
PARAMS = {
    "background_r": "background_color[0]", "background_g": "background_color[1]",
    "background_b": "background_color[2]", "correct_subpixel_offset": "correct_subpixel_offsets",
    **{f"tile_color_{which}_{c}": f"tile_colors[{i}][{j}]"
       for i, which in enumerate(("hi", "lo")) for j, c in enumerate("rgb")},
}

# the tables of named objects: key -> exported array
TABLES = {"gamut_mapping": "pl_gamut_map_functions", "tone_mapping": "pl_tone_map_functions",
          "error_diffusion": "pl_error_diffusion_kernels"}

# enum options: key -> {value name: constant}; a string is a prefix put before the upper-cased name
ENUMS = {
    "tone_map_metadata": "PL_HDR_METADATA_",
    "dither_method": {"blue": "PL_DITHER_BLUE_NOISE", "ordered_lut": "PL_DITHER_ORDERED_LUT",
                      "ordered": "PL_DITHER_ORDERED_FIXED", "white": "PL_DITHER_WHITE_NOISE"},
    "icc_intent": {"auto": "PL_INTENT_AUTO", "perceptual": "PL_INTENT_PERCEPTUAL",
                   "relative": "PL_INTENT_RELATIVE_COLORIMETRIC", "saturation": "PL_INTENT_SATURATION",
                   "absolute": "PL_INTENT_ABSOLUTE_COLORIMETRIC"},
    "cones": "PL_CONE_",
    "deinterlace_algo": "PL_DEINTERLACE_",
    "distort_address_mode": "PL_TEX_ADDRESS_",
    "distort_alpha_mode": "PL_ALPHA_",
    "lut_type": "PL_LUT_",
    "background": "PL_CLEAR_",
    "border": "PL_CLEAR_",
    **{"blend_" + k: {"zero": "PL_BLEND_ZERO", "one": "PL_BLEND_ONE", "alpha": "PL_BLEND_SRC_ALPHA",
                      "one_minus_alpha": "PL_BLEND_ONE_MINUS_SRC_ALPHA"}
       for k in ("src_rgb", "src_alpha", "dst_rgb", "dst_alpha")},
}

# presets: key -> exported object per value name ({} in the pattern = the name)
PRESETS = {
    "preset": "pl_render_{}_params", "deband_preset": "pl_deband_{}_params",
    "sigmoid_preset": "pl_sigmoid_{}_params", "color_adjustment_preset": "pl_color_adjustment_{}",
    "peak_detect_preset": "pl_peak_detect_{}_params", "color_map_preset": "pl_color_map_{}_params",
    "dither_preset": "pl_dither_{}_params", "icc_preset": "pl_icc_{}_params",
    "cone_preset": "pl_vision_{}", "blend_preset": "pl_{}",
    "deinterlace_preset": "pl_deinterlace_{}_params", "distort_preset": "pl_distort_{}_params",
}

TYPES = ("PL_OPT_BOOL", "PL_OPT_INT", "PL_OPT_FLOAT", "PL_OPT_STRING")
KIND_OF_TYPE = ("KIND_BOOL", "KIND_INT", "KIND_FLOAT")


def words(s):
    for a, b in (("[", " "), ("]", ""), (".", " "), ("_", " ")):
        s = s.replace(a, b)
    return s


def struct_of(key):
    """(member of pl_options_t, member of that struct) for a key that lives in a params struct"""
    if key == "blend_against_tiles":    # (of pl_render_params, whatever its first word says)
        return None
    for st, keys in MEMBERS_OF.items():
        if key in keys:
            return st, STRUCTS[st][3].get(key, key)
    for st, (_, toggle, prefix, special) in STRUCTS.items():
        if prefix and key.startswith(prefix) and key != toggle + "_preset":
            return st, special.get(key, key[len(prefix):])
    return None


def describe(e):
    """one option -> (name, kind, value path, target path, choices, table, usage)"""
    key = e["key"]
    toggles = {t: st for st, (_, t, _, _) in STRUCTS.items()}
    if key == "preset":
        return "Preset for all options", "KIND_PRESET_ALL", "params", None, PRESETS[key], None, None
    if key in SCALERS:
        label, usage = SCALERS[key]
        return label, "KIND_SCALER", "params." + key, key, None, None, usage
    for slot, (label, usage) in SCALERS.items():
        if key == slot + "_preset":
            return label + ": custom filter from a built-in one", "KIND_PRESET_SCALER", slot, None, None, None, usage
        part = key[len(slot) + 1:]
        if key.startswith(slot + "_") and part in SCALER_PARTS:
            name = f"{label}: custom {words(SCALER_PARTS[part])}"
            if part in ("kernel", "window"):
                return name, "KIND_NAMED", f"{slot}.{SCALER_PARTS[part]}", None, None, "pl_filter_functions", None
            return name, KIND_OF_TYPE[e["type"]], f"{slot}.{SCALER_PARTS[part]}", None, None, None, None
    if key in toggles:
        st = toggles[key]
        return STRUCTS[st][0], "KIND_TOGGLE", "params." + st, st, None, None, None
    if key in PRESETS:
        st = next(s for s, (_, t, _, _) in STRUCTS.items() if key == t + "_preset")
        return STRUCTS[st][0] + ": preset", "KIND_PRESET", st, None, PRESETS[key], None, None
    where = struct_of(key)
    if where:
        path = f"{where[0]}.{where[1]}"
        name = f"{STRUCTS[where[0]][0]}: {words(where[1])}"
    else:
        path = "params." + PARAMS.get(key, key)
        name = words(PARAMS.get(key, key)).capitalize()
    if key in TABLES:
        return name, "KIND_NAMED", path, None, None, TABLES[key], None
    if key in ENUMS:
        return name, "KIND_ENUM", path, None, ENUMS[key], None, None
    assert e["type"] < 3 and not e["values"], key
    return name, KIND_OF_TYPE[e["type"]], path, None, None, None, None


def number(x):
    return repr(float(np.float32(x))).removesuffix(".0")


def generate():
    entries = json.load(open(LIST))
    choice_arrays, infos, rows = {}, [], []
    for i, e in enumerate(entries):
        name, kind, path, target, choices, table, usage = describe(e)
        assert (choices is not None) == bool(e["values"]), e["key"]
        ch = "NULL"
        if choices is not None:
            items = []
            for v in e["values"]:
                c = choices[v] if isinstance(choices, dict) else \
                    choices.format(v) if "{}" in choices else choices + v.upper()
                items.append(f'{{ "{v}", 0, &{c} }}' if e["preset"] else f'{{ "{v}", {c}, NULL }}')
            body = ", ".join(items)
            ch = choice_arrays.setdefault(body, f"CHOICES_{len(choice_arrays)}")
        infos.append(f"    /* {i:3d} {e['key']} */ {{ {kind}, OFF({path}), SIZE({path}), "
                     f"{'OFF(' + target + ')' if target else '0'}, {ch}, "
                     f"{'TABLE(' + table + ')' if table else 'NULL'}, {usage or '0'} }},")
        rows.append(f'    {{ "{e["key"]}", "{name}", {TYPES[e["type"]]}, {number(e["min"])}, '
                    f'{number(e["max"])}, {str(e["deprecated"]).lower()}, {str(e["preset"]).lower()}, '
                    f'&INFO[{i}] }},')
    out = ["// Written by tools/gen_options_table.py from tests/golden/options_list.json: do not edit.",
           "// CHOICES_n: value names of an enum (name, constant) or a preset list (name, object).", ""]
    for body, ident in choice_arrays.items():
        out.append(f"static const struct choice {ident}[] = {{ {body}, {{0}} }};")
    out += ["", "// kind, value (offset, size), target, choices, table, usage",
            "static const struct opt_info INFO[] = {", *infos, "};", "",
            "// key, name, type, min, max, deprecated, preset, priv",
            "const struct pl_opt_t pl_option_list[] = {", *rows, "    {0},", "};", ""]
    return "\n".join(out)


if __name__ == "__main__":
    text = generate()
    if "--print" in sys.argv:
        sys.stdout.write(text)
    else:
        open(OUT, "w").write(text)
        print(f"wrote {OUT}")

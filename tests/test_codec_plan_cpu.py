"""csrc/codec_plan.h — which packed image every DAC conv weight gets (kind, operand split, tile facts, element count) — built with the host compiler
alone (no HIP) under AddressSanitizer and UBSan and run as a child process (tests/codec_plan_main.cpp prints the plan).  Where a sanitized program
does not link or start, the same program is built and run without the flag.

EXPECTED was written out by hand from the packers this header replaced (ensure_packed, pack_one, pack_one16, pack_one_b3, pack_planes, pack_resunit,
pack_convt_b3 of shim_codec.hip before the image table): one table per distinct layout, per set of dims.  A row is
    layer kind scheme co_t ci_t ns kt transposed elems
(scheme 0 = three bf16 planes, 1 = fp16 hi + lo, 2 = one fp16 plane; the three units of a block share one k7 / k1 row; a fused unit lives under its
k = 7 weight and its k = 1 weight has no image).  Every knob set of ARITH_CASES in tests/test_gpu_dac.py is run, read from that file's text."""
import ast
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "codec_plan_main.cpp")
HEADER = os.path.join(ROOT, "tts.cpp_amd", "csrc", "codec_plan.h")
NO_START = ("error while loading shared libraries", "runtime does not come first in initial library list", "ReserveShadowMemoryRange failed",
            "Shadow memory range interleaves", "LeakSanitizer has encountered a fatal error")

# latent, c0, strides: synth.parler_mini (DAC-44k), tests/golden/upstream_dac_b3.npz, synth.tiny
DIMS = {"dac44k": (1024, 1536, (8, 8, 4, 2)), "upstream_dac_b3": (64, 192, (2, 2)), "tiny": (64, 96, (4, 2))}
# tts_hip_tune key / environment switch -> CodecKnobs fields, as tts_hip_tune and tts_hip_create apply them
LAUNCH_KEYS = {"dac_convt_planes", "dac_wdma"}   # read at launch: the images are the default's
EXACT = {"b3": 0, "fuse": 0, "convt_b3": 0, "planes": 0}


def knobs_of(env, tune):
    k = {}
    if "TTS_HIP_DAC_BF16X3" in env and int(env["TTS_HIP_DAC_BF16X3"]) == 0:
        k.update(EXACT)
    if "TTS_HIP_DAC_SPLIT" in env:
        k["split"] = int(int(env["TTS_HIP_DAC_SPLIT"]) != 0)
    for key, v in tune.items():
        if key == "dac_exact_fp32":
            k.update(EXACT if v else {"b3": 2, "fuse": 1, "convt_b3": 1, "planes": 1})
        elif key in LAUNCH_KEYS:
            continue
        else:
            assert key.startswith("dac_"), key
            k[key[4:]] = int(v)
    return k


# which table of EXPECTED a case's layout is
TABLE_OF = {"default_fp16_hi_lo": "default", "bf16x3": "bf16x3", "bf16x3_by_env": "bf16x3", "exact_fp32": "exact_fp32", "exact_fp32_by_key": "exact_fp32",
            "units_unfused": "units_unfused", "convt_fp32": "convt_fp32", "no_planes": "no_planes", "tap_pairs": "tap_pairs", "convt_fp32_input": "default",
            "units_weights_by_registers": "default", "units_unfused_conv1_mfma": "units_unfused_conv1_mfma"}


def arith_cases():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_dac.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "ARITH_CASES":
            return [(ast.literal_eval(e.elts[0]), ast.literal_eval(e.elts[1]), ast.literal_eval(e.elts[2])) for e in node.value.elts]
    raise AssertionError("ARITH_CASES not found in tests/test_gpu_dac.py")


EXPECTED = {
    "dac44k": {
        "default": """
            init planes 1 64 16 7 7 0 22020096
            b0.convt convt_planes 1 32 16 0 16 1 37748736
            b0.k7 planes 1 64 16 7 7 0 8257536
            b0.k1 planes 1 256 16 1 1 0 1179648
            b1.convt convt_planes 1 32 16 0 16 1 9437184
            b1.k7 planes 1 64 16 7 7 0 2064384
            b1.k1 planes 1 128 16 1 1 0 294912
            b2.convt convt_planes 1 64 16 0 8 1 1179648
            b2.k7 unit_tap 1 192 16 0 7 0 675840
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt convt_planes 1 96 16 0 4 1 147456
            b3.k7 unit_tap 1 96 16 0 7 0 184320
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "bf16x3": """
            init planes 0 64 16 7 7 0 33030144
            b0.convt convt_planes 0 32 16 0 16 1 56623104
            b0.k7 planes 0 64 16 7 7 0 12386304
            b0.k1 planes 0 256 16 1 1 0 1769472
            b1.convt convt_planes 0 32 16 0 16 1 14155776
            b1.k7 planes 0 64 16 7 7 0 3096576
            b1.k1 planes 0 128 16 1 1 0 442368
            b2.convt convt_planes 0 64 16 0 8 1 1769472
            b2.k7 unit_tap 0 192 16 0 7 0 1013760
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt convt_planes 0 96 16 0 4 1 221184
            b3.k7 unit_tap 0 96 16 0 7 0 276480
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "exact_fp32": """
            init f32_tile 0 128 4 0 7 0 11010048
            b0.convt f32_tile 0 64 8 0 16 1 18874368
            b0.k7 f32_tile 0 128 4 0 7 0 4128768
            b0.k1 f32_tile 0 128 16 0 1 0 589824
            b1.convt f32_tile 0 64 8 0 16 1 4718592
            b1.k7 f32_tile 0 128 4 0 7 0 1032192
            b1.k1 f32_tile 0 128 16 0 1 0 147456
            b2.convt f32_tile 0 64 8 0 8 1 589824
            b2.k7 f32_tile 0 64 4 0 7 0 258048
            b2.k1 f32_direct 0 192 16 0 1 0 36864
            b3.convt f32_tile 0 96 8 0 4 1 73728
            b3.k7 f32_tile 0 96 4 0 7 0 64512
            b3.k1 f32_direct 0 96 16 0 1 0 9216
        """,
        "units_unfused": """
            init planes 1 64 16 7 7 0 22020096
            b0.convt convt_planes 1 32 16 0 16 1 37748736
            b0.k7 planes 1 64 16 7 7 0 8257536
            b0.k1 planes 1 256 16 1 1 0 1179648
            b1.convt convt_planes 1 32 16 0 16 1 9437184
            b1.k7 planes 1 64 16 7 7 0 2064384
            b1.k1 planes 1 128 16 1 1 0 294912
            b2.convt convt_planes 1 64 16 0 8 1 1179648
            b2.k7 b3 1 64 8 0 7 0 589824
            b2.k1 f32_direct 0 192 16 0 1 0 36864
            b3.convt convt_planes 1 96 16 0 4 1 147456
            b3.k7 b3 1 96 8 0 7 0 147456
            b3.k1 f32_direct 0 96 16 0 1 0 9216
        """,
        "convt_fp32": """
            init planes 1 64 16 7 7 0 22020096
            b0.convt f32_tile 0 64 8 0 16 1 18874368
            b0.k7 planes 1 64 16 7 7 0 8257536
            b0.k1 planes 1 256 16 1 1 0 1179648
            b1.convt f32_tile 0 64 8 0 16 1 4718592
            b1.k7 planes 1 64 16 7 7 0 2064384
            b1.k1 planes 1 128 16 1 1 0 294912
            b2.convt f32_tile 0 64 8 0 8 1 589824
            b2.k7 unit_tap 1 192 16 0 7 0 675840
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt f32_tile 0 96 8 0 4 1 73728
            b3.k7 unit_tap 1 96 16 0 7 0 184320
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "no_planes": """
            init b3 1 64 8 0 7 0 25165824
            b0.convt convt_planes 1 32 16 0 16 1 37748736
            b0.k7 b3 1 64 8 0 7 0 9437184
            b0.k1 f32_tile 0 128 16 0 1 0 589824
            b1.convt convt_planes 1 32 16 0 16 1 9437184
            b1.k7 b3 1 64 8 0 7 0 2359296
            b1.k1 f32_tile 0 128 16 0 1 0 147456
            b2.convt convt_planes 1 64 16 0 8 1 1179648
            b2.k7 unit_tap 1 192 16 0 7 0 675840
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt convt_planes 1 96 16 0 4 1 147456
            b3.k7 unit_tap 1 96 16 0 7 0 184320
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "tap_pairs": """
            init planes 1 64 8 4 7 0 25165824
            b0.convt convt_planes 1 32 16 0 16 1 37748736
            b0.k7 planes 1 64 8 4 7 0 9437184
            b0.k1 planes 1 256 16 1 1 0 1179648
            b1.convt convt_planes 1 32 16 0 16 1 9437184
            b1.k7 planes 1 64 8 4 7 0 2359296
            b1.k1 planes 1 128 16 1 1 0 294912
            b2.convt convt_planes 1 64 16 0 8 1 1179648
            b2.k7 unit_pair 0 192 8 0 7 0 1013760
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt convt_planes 1 96 16 0 4 1 147456
            b3.k7 unit_pair 0 96 8 0 7 0 276480
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "units_unfused_conv1_mfma": """
            init planes 1 64 16 7 7 0 22020096
            b0.convt convt_planes 1 32 16 0 16 1 37748736
            b0.k7 planes 1 64 16 7 7 0 8257536
            b0.k1 planes 1 256 16 1 1 0 1179648
            b1.convt convt_planes 1 32 16 0 16 1 9437184
            b1.k7 planes 1 64 16 7 7 0 2064384
            b1.k1 planes 1 128 16 1 1 0 294912
            b2.convt convt_planes 1 64 16 0 8 1 1179648
            b2.k7 b3 1 64 8 0 7 0 589824
            b2.k1 f32_tile 0 64 16 0 1 0 36864
            b3.convt convt_planes 1 96 16 0 4 1 147456
            b3.k7 b3 1 96 8 0 7 0 147456
            b3.k1 f32_tile 0 96 16 0 1 0 9216
        """,
        "f16_planes": """
            init planes 2 64 16 7 7 0 11010048
            b0.convt convt_planes 2 32 16 0 16 1 18874368
            b0.k7 planes 2 64 16 7 7 0 4128768
            b0.k1 planes 2 256 16 1 1 0 589824
            b1.convt convt_planes 2 32 16 0 16 1 4718592
            b1.k7 planes 2 64 16 7 7 0 1032192
            b1.k1 planes 2 128 16 1 1 0 147456
            b2.convt convt_planes 2 64 16 0 8 1 589824
            b2.k7 unit_tap 2 192 16 0 7 0 337920
            b2.k1 none 0 0 0 0 0 0 0
            b3.convt convt_planes 2 96 16 0 4 1 73728
            b3.k7 unit_tap 2 96 16 0 7 0 92160
            b3.k1 none 0 0 0 0 0 0 0
        """,
        "f16_tiles": """
            init f16_tile 0 128 16 0 7 0 11010048
            b0.convt f16_tile 0 64 16 0 16 1 18874368
            b0.k7 f16_tile 0 128 16 0 7 0 4128768
            b0.k1 f16_tile 0 128 32 0 1 0 589824
            b1.convt f16_tile 0 64 16 0 16 1 4718592
            b1.k7 f16_tile 0 128 16 0 7 0 1032192
            b1.k1 f16_tile 0 128 32 0 1 0 147456
            b2.convt f16_tile 0 64 16 0 8 1 589824
            b2.k7 f16_tile 0 64 16 0 7 0 258048
            b2.k1 f16_tile 0 64 32 0 1 0 36864
            b3.convt f16_tile 0 96 16 0 4 1 73728
            b3.k7 f16_tile 0 96 16 0 7 0 64512
            b3.k1 f16_tile 0 96 32 0 1 0 9216
        """,
    },
    "upstream_dac_b3": {
        "default": """
            init b3 1 64 8 0 7 0 196608
            b0.convt convt_planes 1 96 16 0 4 1 147456
            b0.k7 unit_tap 1 96 16 0 7 0 184320
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "bf16x3": """
            init b3 0 64 8 0 7 0 294912
            b0.convt convt_planes 0 96 16 0 4 1 221184
            b0.k7 unit_tap 0 96 16 0 7 0 276480
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "exact_fp32": """
            init f32_tile 0 64 4 0 7 0 86016
            b0.convt f32_tile 0 96 8 0 4 1 73728
            b0.k7 f32_tile 0 96 4 0 7 0 64512
            b0.k1 f32_direct 0 96 16 0 1 0 9216
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "units_unfused": """
            init b3 1 64 8 0 7 0 196608
            b0.convt convt_planes 1 96 16 0 4 1 147456
            b0.k7 b3 1 96 8 0 7 0 147456
            b0.k1 f32_direct 0 96 16 0 1 0 9216
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "convt_fp32": """
            init b3 1 64 8 0 7 0 196608
            b0.convt f32_tile 0 96 8 0 4 1 73728
            b0.k7 unit_tap 1 96 16 0 7 0 184320
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "no_planes": """
            init b3 1 64 8 0 7 0 196608
            b0.convt convt_planes 1 96 16 0 4 1 147456
            b0.k7 unit_tap 1 96 16 0 7 0 184320
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "tap_pairs": """
            init b3 1 64 8 0 7 0 196608
            b0.convt convt_planes 1 96 16 0 4 1 147456
            b0.k7 unit_pair 0 96 8 0 7 0 276480
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "units_unfused_conv1_mfma": """
            init b3 1 64 8 0 7 0 196608
            b0.convt convt_planes 1 96 16 0 4 1 147456
            b0.k7 b3 1 96 8 0 7 0 147456
            b0.k1 f32_tile 0 96 16 0 1 0 9216
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "f16_planes": """
            init f16_tile 0 64 16 0 7 0 86016
            b0.convt convt_planes 2 96 16 0 4 1 73728
            b0.k7 unit_tap 2 96 16 0 7 0 92160
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "f16_tiles": """
            init f16_tile 0 64 16 0 7 0 86016
            b0.convt f16_tile 0 96 16 0 4 1 73728
            b0.k7 f16_tile 0 96 16 0 7 0 64512
            b0.k1 f16_tile 0 96 32 0 1 0 9216
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
    },
    "tiny": {
        "default": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "bf16x3": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "exact_fp32": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "units_unfused": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "convt_fp32": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "no_planes": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "tap_pairs": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "units_unfused_conv1_mfma": """
            init f32_tile 0 96 4 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "f16_planes": """
            init f16_tile 0 96 16 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
        "f16_tiles": """
            init f16_tile 0 96 16 0 7 0 43008
            b0.convt none 0 0 0 0 0 0 0
            b0.k7 none 0 0 0 0 0 0 0
            b0.k1 none 0 0 0 0 0 0 0
            b1.convt none 0 0 0 0 0 0 0
            b1.k7 none 0 0 0 0 0 0 0
            b1.k1 none 0 0 0 0 0 0 0
        """,
    },
}


def _build(cxx, exe, sanitize):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    return subprocess.run(cmd + [SRC, "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++)")
    exe = str(tmp_path_factory.mktemp("codec_plan") / "codec_plan_main")
    probe = ["1024", "1536", "8,8,4,2"]
    built = _build(cxx, exe, sanitize=True)
    ran = subprocess.run([exe] + probe, capture_output=True, text=True) if built.returncode == 0 else None
    # unusable: the sanitized program does not link, or the loader / the runtime's start-up says it cannot run here.  Any other non-zero exit
    # (a report of any sanitizer) is a failure of the test that meets it
    if built.returncode != 0 or (ran.returncode != 0 and any(m in ran.stderr for m in NO_START)):
        built = _build(cxx, exe, sanitize=False)
        assert built.returncode == 0, built.stderr
    return exe


def _plan(exe, dims, knobs):
    latent, c0, strides = DIMS[dims]
    ran = subprocess.run([exe, str(latent), str(c0), ",".join(map(str, strides))] + [f"{k}={v}" for k, v in sorted(knobs.items())], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    return ran.stdout.split("\n")[:-1]


def _rows(text):
    return [line.strip() for line in text.strip().split("\n")]


def test_header_has_no_hip_in_it():
    includes = [line.split()[1] for line in open(HEADER).read().splitlines() if line.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>", "<string.h>"], includes


def test_arith_cases_are_all_mapped():
    assert sorted(TABLE_OF) == sorted(c[0] for c in arith_cases())


@pytest.mark.parametrize("dims", list(DIMS))
def test_default_and_every_arith_case(program, dims):
    assert _plan(program, dims, {}) == _rows(EXPECTED[dims]["default"])
    for name, env, tune in arith_cases():
        assert _plan(program, dims, knobs_of(env, tune)) == _rows(EXPECTED[dims][TABLE_OF[name]]), name


@pytest.mark.parametrize("dims", list(DIMS))
def test_f16_tensors_on_planes_and_on_tiles(program, dims):
    assert _plan(program, dims, {"f16": 1, "f16_planes": 1}) == _rows(EXPECTED[dims]["f16_planes"])
    assert _plan(program, dims, {"f16": 1, "f16_planes": 0}) == _rows(EXPECTED[dims]["f16_tiles"])


@pytest.mark.parametrize("dims", list(DIMS))
def test_valu_flag_plans_no_image(program, dims):
    assert all(row.split()[1] == "none" for row in _plan(program, dims, {"valu": 1}))

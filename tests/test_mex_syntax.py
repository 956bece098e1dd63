"""The MATLAB-side binding (matlab/) never meets MATLAB in this image; this is what CAN be checked on a CPU:
  * the mex gateway is type-correct C++ against the documented MEX API (a declarations-only tests/mex_decl/mex.h) and
    against include/aps.h - every C-ABI call it makes has the right arity and types;
  * every command string a shadowing .m wrapper sends exists in the gateway's dispatcher;
  * every .m file is structurally sound (balanced function/end blocks, a single main function named like the file) and
    shadows a function that really exists under the same name in the reference tree layout listed in INTEGRATION.md."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATLAB = os.path.join(ROOT, "matlab")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_mex_gateway_is_type_correct_against_the_mex_api_and_aps_h():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "tests", "mex_decl"), os.path.join(MATLAB, "aps_mex.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _gateway_commands():
    src = open(os.path.join(MATLAB, "aps_mex.cpp")).read()
    return set(re.findall(r'cmd == "([a-z0-9_]+)"', src))


def test_every_wrapper_command_exists_in_the_gateway():
    cmds = _gateway_commands()
    assert {"sift_extract", "match_features", "render", "image_warp", "crop_nonzero_bbox", "multiband_blend"} <= cmds
    used = set()
    for f in os.listdir(MATLAB):
        if f.endswith(".m"):
            used |= set(re.findall(r"aps_mex\('([a-z0-9_]+)'", open(os.path.join(MATLAB, f)).read()))
    assert used and used <= cmds, used - cmds


def _strip(code):
    out = []
    for line in code.splitlines():
        line = re.sub(r"'[^']*'", "''", line)       # string literals
        line = line.split("%")[0]                    # comments
        out.append(line)
    return "\n".join(out)


def test_m_files_are_structurally_sound():
    openers = re.compile(r"\b(function|if|for|while|switch|try|parfor|arguments)\b")
    for f in sorted(os.listdir(MATLAB)):
        if not f.endswith(".m"):
            continue
        code = _strip(open(os.path.join(MATLAB, f)).read())
        m = re.search(r"^\s*function\s+(?:\[[^\]]*\]\s*=\s*|\w+\s*=\s*)?(\w+)", code, re.M)
        assert m and m.group(1) == f[:-2], f"{f}: main function must be named like the file"
        n_open = len(openers.findall(code))
        n_end = len(re.findall(r"\bend\b", re.sub(r"\([^()]*\bend\b[^()]*\)", "()", code)))  # x(end) is an index, not a block end
        assert n_open == n_end, f"{f}: {n_open} block openers vs {n_end} ends"
        assert code.count("(") == code.count(")") and code.count("[") == code.count("]"), f


def test_shadows_cover_the_operator_table_of_survey_8b():
    have = {f[:-2] for f in os.listdir(MATLAB) if f.endswith(".m")}
    need = {"getFeaturePoints", "featureMatchingPairwise", "matchFeaturesScratch", "flann_knn_win",
            "nearest2HammingExhaustiveMEX", "nearest2HammingExhaustiveOMPMEX", "estimateTransformationRANSAC",
            "estimateTransformationMLESAC", "renderPanorama", "multiBandBlending", "linearBlending", "imageWarp",
            "featureMatchingGlobal", "imageMatching"}
    assert need <= have, need - have


def _calls(src, name_re=r"aps_[a-z0-9_]+"):
    """(entry point, argument text) of every call `aps_xxx( ... )` in a source text, parentheses balanced."""
    out = []
    for m in re.finditer(r"\b(" + name_re + r")\s*\(", src):
        depth, i = 1, m.end()
        while depth and i < len(src):
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        out.append((m.group(1), src[m.end():i - 1]))
    return out


LAYOUT_CONSTANTS = ("APS_IMG_U8_MATLAB", "APS_COLMAJOR")


def test_every_matlab_layout_call_of_the_gateway_has_a_layout_test():
    """The gateway is the only caller of the MATLAB-side layout branches and never runs here.  Every entry point it calls with
    APS_IMG_U8_MATLAB or APS_COLMAJOR must be called with that constant in tests/test_abi_layouts_gpu.py (a plain text check:
    the entry point's name and the constant inside one test function), so a new gateway command with a MATLAB layout fails
    the CPU suite until it has a layout test."""
    gateway = open(os.path.join(MATLAB, "aps_mex.cpp")).read()
    need = {(name, c) for name, args in _calls(gateway) for c in LAYOUT_CONSTANTS if re.search(r"\b" + c + r"\b", args)}
    assert {("aps_sift_extract", "APS_IMG_U8_MATLAB"), ("aps_sift_extract", "APS_COLMAJOR"), ("aps_render", "APS_IMG_U8_MATLAB"),
            ("aps_knn_global", "APS_COLMAJOR"), ("aps_crop_nonzero_bbox", "APS_IMG_U8_MATLAB")} <= need
    tests = open(os.path.join(ROOT, "tests", "test_abi_layouts_gpu.py")).read()
    functions = re.split(r"^(?=def |@pytest)", tests, flags=re.M)  # one chunk per top-level function (helpers included)
    # a test reaches an entry point either directly (`lib.aps_x`) or through a helper of this module that it names
    helpers = {m.group(1): chunk for chunk in functions for m in [re.match(r"def (_[a-z0-9_]+)\(", chunk)] if m}
    have = set()
    for chunk in functions:
        if not re.search(r"^def test_", chunk, re.M):
            continue
        text = chunk + "".join(body for name, body in helpers.items() if re.search(r"\b" + name + r"\(", chunk))
        for name in set(re.findall(r"lib\.(aps_[a-z0-9_]+)", text)) | set(re.findall(r'"(aps_[a-z0-9_]+)"', text)):
            for c in LAYOUT_CONSTANTS:
                if re.search(r"\b" + c + r"\b", text):
                    have.add((name, c))
    assert need <= have, sorted(need - have)

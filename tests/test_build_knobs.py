"""The kernel sources carry no compile-time experiment knobs: the only VIP_* names the
preprocessor tests are the translation-unit selectors, the quick-build selectors and the
diagnostic stamp builds, and the build files define nothing but the translation-unit
selectors. (Settled tunables are constexpr constants; measurements live in DESIGN.md.)"""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "various_image_processings_amd" / "csrc"

TU_SELECTORS = {"VIP_BIL_JOINT", "VIP_BIL_FMA", "VIP_ADA_FMA"}
KEPT = TU_SELECTORS | {"VIP_ONLY_R7", "VIP_GF_ONLY_R2", "VIP_STAMPS", "VIP_GF_STAMPS"}

NAME = r"VIP_[A-Z0-9_]+"


def _logical_lines(text):
    return text.replace("\\\n", " ").splitlines()


def _tested_names(text):
    names = set()
    for line in _logical_lines(text):
        m = re.match(r"\s*#\s*(ifdef|ifndef|if|elif)\b(.*)", line)
        if not m:
            continue
        rest = m.group(2).split("//")[0]
        names.update(re.findall(NAME, rest))
    return names


def test_preprocessor_tests_only_the_kept_names():
    sources = sorted(p for ext in ("*.hip", "*.hpp", "*.cpp") for p in CSRC.glob(ext))
    assert sources, "no kernel sources found"
    found = {}
    for p in sources:
        for n in _tested_names(p.read_text()):
            found.setdefault(n, []).append(p.name)
    assert set(found) == KEPT, {n: f for n, f in found.items() if n not in KEPT} or sorted(KEPT - set(found))


def test_build_files_define_only_the_translation_unit_selectors():
    make = (CSRC / "Makefile").read_text()
    defined = set(re.findall(r"-D(%s)" % NAME, make))
    cmake = (ROOT / "CMakeLists.txt").read_text()
    defined |= set(re.findall(r"-D(%s)" % NAME, cmake))
    # vip_variant(<target> <source> <definitions...>) and any target_compile_definitions / add_definitions
    for args in re.findall(r"\bvip_variant\(\s*\S+\s+\S+([^)]*)\)", cmake):
        defined |= set(re.findall(NAME, args))
    for args in re.findall(r"\b(?:target_compile_definitions|add_compile_definitions|add_definitions)\(([^)]*)\)", cmake):
        defined |= set(re.findall(NAME, args))
    assert defined == TU_SELECTORS, sorted(defined ^ TU_SELECTORS)

"""The product is built from one version of the kernels: no compile-time A/B switch is left (CPU).

Round 11 removed every structural `YK_*` switch of ykgpu_render.hip, keeping the branch the product
was built with (profiles/r11_knobs/README.md lists them, the value kept and the evidence).  Two
things keep that true: the product's Makefile recipes define nothing but `YK_SPLIT`, and none of
the removed names comes back into the sources.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uecraytracing_amd", "csrc")

PRODUCT_TARGETS = ("ykgpu_render.o", "ykgpu_render_f32.o", "yk_denoise.o", "yk_features.o", "libykgpu.so")

REMOVED = [
    "YK_NODE_BF",
    "YK_VISIT_UNSWITCH",
    "YK_SLAB_PAIRS",
    "YK_SLAB_PAIRS_F64",
    "YK_SLAB_PAIRS_F32",
    "YK_NEAR_CLAMP",
    "YK_CULL_BLOCK",
    "YK_CAND_PACK",
    "YK_CAND_HD",
    "YK_CAND_RSQ",
    "YK_RA_FROM_IA",
    "YK_STACK_EXACT",
    "YK_DIEL_PRE",
    "YK_UNWIND_FAST",
    "YK_CLAIM_ARGS",
    "YK_WG_HOLD",
    "YK_RENDER_PRIO",
    "YK_WAVES_PER_EU",
    "YK_SINGLE_VGPRS",
    "YK_WALK_SENS",
    "YK_WALK_ILP_INLINE",
    "YK_LENS_DEFER",
    "YK_INFLIGHT_DEEP",
    "YK_SCHED_SLOW",
    "YK_RED_PRIO",
    "YK_WARM_TRIM",
    "kInflightDeep",
    "kSchedSlow",
    "kLensDefer",
]


def recipes():
    """target file name -> its recipe lines, of every rule of the Makefile"""
    out, cur = {}, None
    for line in open(os.path.join(CSRC, "Makefile")).read().split("\n"):
        m = re.match(r"^\$\(LIB\)/([^\s:]+)\s*:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif line.startswith("\t") and cur:
            out[cur].append(line)
        elif line.strip() and not line.startswith("#"):
            cur = None
    return out


def test_product_recipes_define_only_yk_split():
    rules = recipes()
    for target in PRODUCT_TARGETS:
        assert rules.get(target), f"the Makefile has no recipe for {target}"
        defs = re.findall(r"-DYK_\S*", "\n".join(rules[target]))
        assert set(defs) <= {"-DYK_SPLIT=1", "-DYK_SPLIT=2"}, (target, defs)
    # the two render units are the ones YK_SPLIT makes
    assert re.findall(r"-DYK_\S*", "\n".join(rules["ykgpu_render.o"])) == ["-DYK_SPLIT=1"]
    assert re.findall(r"-DYK_\S*", "\n".join(rules["ykgpu_render_f32.o"])) == ["-DYK_SPLIT=2"]


def test_no_removed_switch_in_the_sources():
    found = []
    for dirpath, _, files in os.walk(CSRC):
        for f in files:
            text = open(os.path.join(dirpath, f), errors="replace").read()
            found += [(os.path.relpath(os.path.join(dirpath, f), ROOT), name) for name in REMOVED
                      if name in text]
    assert not found, found

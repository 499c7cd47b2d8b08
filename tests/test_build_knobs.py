"""The product is built from one version of the kernels: no compile-time A/B switch is left (CPU).

Round 11 removed every structural `YK_*` switch of the render kernels, keeping the branch the
product was built with (profiles/r11_knobs/README.md lists them, the value kept and the evidence).
Round 12 took the two path kernels out of ykgpu_render.hip into units of their own, each source
file compiled once (profiles/r12_split/README.md), which removed `YK_SPLIT` too.  Round 13 split the rest of that
file into context, pipeline, film, group and math units behind yk_host_internal.hpp
(profiles/r13_units/README.md), which removed the film view the denoise and feature units worked
through and their copies of the error macro.  Three things keep that true: the
product's Makefile recipes define no `YK_*` at all, none of the removed names comes back into the
sources, and a test variant compiles one unit with its switch and links the product's other objects:
a unit without a path kernel, whose switch replaces one constant of its host code or, for the sky
blocks' lazy-word limit and the query kernels' stack capacity, of one of its own small kernels'
launches (tests/test_gpu_fallbacks.py runs those two).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uecraytracing_amd", "csrc")

# the library's units: one object each (the Makefile's HIP_UNITS and CXX_UNITS)
HIP_UNITS = ("yk_render_f64", "yk_render_f32", "yk_pipeline", "yk_context", "yk_film", "yk_group", "yk_math",
             "yk_denoise", "yk_features")
CXX_UNITS = ("yk_host", "yk_bvh")
# the rules that make the product: the two object patterns and the link
PRODUCT_TARGETS = ("%.o", "libykgpu.so")
# target -> (its switch, the one unit that reads it, the Makefile variable of the product's other objects)
TEST_VARIANTS = {"abl/libykgpu_retry%.so": ("YK_RETRY_CAP_FORCE", "yk_pipeline", "REST_RETRY"),
                 "abl/libykgpu_stack%.so": ("YK_STACK_CAP_FORCE", "yk_context", "REST_STACK"),
                 "abl/libykgpu_skylazy%.so": ("YK_SKY_LAZY_FORCE", "yk_pipeline", "REST_RETRY"),
                 "abl/libykgpu_qstack%.so": ("YK_QUERY_STACK_FORCE", "yk_features", "REST_QSTACK")}
# the instances `make all` builds (the Makefile's TESTVARIANTS)
TEST_VARIANT_FILES = ["abl/libykgpu_retry64.so", "abl/libykgpu_retry0.so", "abl/libykgpu_stack5.so",
                      "abl/libykgpu_skylazy8.so", "abl/libykgpu_qstack2.so"]

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
    "YK_SPLIT",
    "yk_split_f32_kernel",
    "yk_film_view",
    "yk_film_view_of",
    "yk_film_fail",
    "YKD_HIP",
    "YKF_HIP",
]


def makefile():
    return open(os.path.join(CSRC, "Makefile")).read().split("\n")


def recipes():
    """target file name -> the recipe lines of its rules (a target-specific variable counts as a
    line of its target), of every rule of the Makefile for a file under $(LIB)"""
    out, cur = {}, None
    for line in makefile():
        m = re.match(r"^\$\(LIB\)/([^\s:]+)\s*:(.*)$", line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
            if re.match(r"^\s*\w+\s*[:+?]?=", m.group(2)):
                out[cur].append(m.group(2))
        elif line.startswith("\t") and cur:
            out[cur].append(line)
        elif line.strip() and not line.startswith("#"):
            cur = None
    return out


def variable(name):
    for line in makefile():
        m = re.match(r"^%s\s*[:+?]?=(.*)$" % re.escape(name), line)
        if m:
            return m.group(1).split("#")[0].split()
    raise AssertionError(f"the Makefile sets no {name}")


def test_units_are_the_makefiles():
    assert tuple(variable("HIP_UNITS")) == HIP_UNITS and tuple(variable("CXX_UNITS")) == CXX_UNITS
    for u in HIP_UNITS:
        assert os.path.exists(os.path.join(CSRC, u + ".hip")), u
    for u in CXX_UNITS:
        assert os.path.exists(os.path.join(CSRC, u + ".cpp")), u
    # every .hip file is a unit of the library, and the file the round-13 split dissolved is gone
    assert sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip")) == sorted(HIP_UNITS)
    assert not os.path.exists(os.path.join(CSRC, "ykgpu_render.hip"))


def test_product_recipes_define_no_yk_switch():
    rules = recipes()
    for target in PRODUCT_TARGETS:
        assert rules.get(target), f"the Makefile has no recipe for {target}"
    # no rule for a product file, and no flag variable, defines a YK_* macro
    for target, lines in rules.items():
        if target not in TEST_VARIANTS:
            assert not re.findall(r"-DYK_\S*", "\n".join(lines)), (target, lines)
    for name in ("CXXFLAGS", "HIPFLAGS", "DEPFLAGS", "DEFS"):
        assert not [w for w in variable(name) if w.startswith("-D")], name
    # every unit is compiled by one of the two pattern rules, once: no unit has a rule of its own
    # with a recipe, and each pattern's recipe is one compile
    compiles = [l for l in rules["%.o"] if " -c " in l]
    assert len(compiles) == 2 and len(rules["%.o"]) == 4, rules["%.o"]
    for u in HIP_UNITS + CXX_UNITS:
        assert not [l for l in rules.get(u + ".o", []) if l.startswith("\t")], u
    # the one per-unit flag: the FP32 path kernel's scheduler
    assert rules["yk_render_f32.o"] == [" UNITFLAGS = -mllvm --amdgpu-sched-strategy=max-ilp"]
    assert [t for t in rules if t.endswith(".o") and rules[t] and t != "%.o"] == ["yk_render_f32.o"]


def test_test_variants_compile_one_host_unit_and_link_the_products_objects():
    rules = recipes()
    assert variable("OBJS") == ["$(HIP_UNITS:%=$(LIB)/%.o)", "$(CXX_UNITS:%=$(LIB)/%.o)"]
    for target, (switch, unit, rest) in TEST_VARIANTS.items():
        assert variable(rest) == ["$(filter-out", "$(LIB)/%s.o,$(OBJS))" % unit]
        lines = [l for l in rules[target] if not l.strip().startswith("@")]
        compiles = [l for l in lines if " -c " in l]
        links = [l for l in lines if " -shared " in l]
        assert len(compiles) == 1 and len(links) == 1 and len(lines) == 2, lines
        # the one compile: the unit that reads the switch, with that switch and nothing else defined
        assert re.findall(r"-D\S*", compiles[0]) == [f"-D{switch}=$*"], compiles[0]
        assert re.fullmatch(r"YK_\w+_FORCE", switch)
        assert compiles[0].split()[-1] == unit + ".hip"
        obj = compiles[0].split()[compiles[0].split().index("-o") + 1]
        # the link: that object and the product's other objects, unchanged
        assert links[0].split()[links[0].split().index("$@") + 1:] == [obj, "$(%s)" % rest], links[0]
        # the switch is host code of its unit alone, a unit without a render kernel
        for f in os.listdir(CSRC):
            text = open(os.path.join(CSRC, f), errors="replace").read()
            if f not in (unit + ".hip", "Makefile"):
                assert switch not in text, f
            if f not in [u + ".hip" for _, u, _ in TEST_VARIANTS.values()] + ["Makefile"]:
                assert "_CAP_FORCE" not in text, f
                assert not re.search(r"YK_\w+_FORCE", text), f
        main = open(os.path.join(CSRC, unit + ".hip")).read()
        assert switch in main
        # ... and the unit reads no switch but its own (yk_pipeline.hip has two, each with its variant)
        own = {s for s, u, _ in TEST_VARIANTS.values() if u == unit}
        assert [w for w in re.findall(r"YK_\w+_CAP_FORCE", main) if w not in own] == [], unit
        assert set(re.findall(r"YK_\w+_FORCE", main)) == own, unit
        assert not re.search(r"void\s+yk_render_\w+\s*\(", main)
        assert "#include \"yk_path.hpp\"" not in main


def test_make_all_builds_every_test_variant():
    words = []
    lines = makefile()
    k = next(i for i, l in enumerate(lines) if re.match(r"^TESTVARIANTS\s*=", l))
    while True:  # (the variable's value, continuation lines included)
        words += lines[k].rstrip("\\").split("=")[-1].split()
        if not lines[k].endswith("\\"):
            break
        k += 1
    assert words == ["$(LIB)/" + f for f in TEST_VARIANT_FILES]
    assert [l for l in lines if l.startswith("all:")] == ["all: $(LIB)/libykgpu.so $(LIB)/raytrace $(TESTVARIANTS)"]
    for f in TEST_VARIANT_FILES:  # every instance is one of the pattern rules
        assert [t for t in TEST_VARIANTS if re.fullmatch(t.replace("%", r"\d+"), f)], f


def test_the_query_kernels_share_one_closest_hit():
    """The checked-stack FP64 visit of DESIGN.md §4 is written once, in yk_query.hpp: no other header
    of the unit yk_features.hip stores the stack's sentinel, defines a slot test, states the tie
    rule or writes the ordered scan's loop (the unit's own file keeps the pinhole pass's staged scan)."""
    main = open(os.path.join(CSRC, "yk_features.hip")).read()
    # the unit's query headers: what it includes at its end, after the stack switch
    headers = re.findall(r'#include "(yk_\w+\.hpp)"', main[main.index("kYkQueryStackForce = 0;"):])
    assert headers == ["yk_query.hpp", "yk_cast.hpp", "yk_radiance.hpp", "yk_gather.hpp", "yk_features_sampled.hpp"]
    once = {"the sentinel's store": r"=\s*ykbvh::kEmptyLeaf\s*;",
            "the slot test": r"#define\s+YK_\w*SLOT\b",
            "the tie rule": re.escape("r == best && (int)id > best_id"),
            "the ordered loop": r"root < \w[\w.]* \|\| \w+ < root"}
    for what, pattern in once.items():
        found = {f: len(re.findall(pattern, open(os.path.join(CSRC, f)).read())) for f in headers}
        want = 2 if what == "the ordered loop" else 1  # (the loop tests each of a sphere's two roots)
        assert found == {f: (want if f == "yk_query.hpp" else 0) for f in headers}, (what, found)
    # ... and the unit's own file has the pinhole pass's loop alone
    assert len(re.findall(once["the ordered loop"], main)) == 2
    assert not [w for w in list(once)[:3] if re.search(once[w], main)]


def test_no_removed_switch_in_the_sources():
    found = []
    for dirpath, _, files in os.walk(CSRC):
        for f in files:
            text = open(os.path.join(dirpath, f), errors="replace").read()
            found += [(os.path.relpath(os.path.join(dirpath, f), ROOT), name) for name in REMOVED
                      if name in text]
    assert not found, found

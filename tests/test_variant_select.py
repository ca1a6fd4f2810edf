"""Which compiled build of render_kernel a launch takes: select_variant and the variant table of csrc/hip/pt_variant.h -- the one statement of
the rule, called by launch_render and by the CPU emulator -- against an independent restatement of the rule written out here.  No GPU: the
emulator library exports the function (tests/emu/pt_emu.cpp emu_select_variant).

The restatement below is a transcription of the launcher as it stood when the rule still lived in launch_render and in the fifteen launch_set_*
functions of the instance files (one Python function per launch_set_* function, the fall-through calls included).  It is text, not derived from
the table: a row or a branch that changes in pt_variant.h fails here until this file is changed with it, on purpose."""
import itertools
import os

import pytest

from conftest import ROOT
import support                          # noqa: F401  (its import puts tests/emu, where emu_api lives, on the path)

# include/prt_types.h
LIGHT, DIFF, COND, DIEL, COAT, ROUGH_COND, ROUGH_DIEL = 1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 10, 1 << 11
BECKMANN, PHONG, GGX = 1 << 0, 1 << 1, 1 << 2
# the PT_MATS_* bits of a build's MATS
SDF, VIEW, PICK, ENVIS, FILTER, DIST_SHIFT = 0x80000000, 0x40000000, 0x20000000, 0x10000000, 0x00800000, 24

LD = LIGHT | DIFF
CO = LIGHT | DIFF | COAT
RC = LIGHT | DIFF | ROUGH_COND
RD = LIGHT | DIFF | DIEL | ROUGH_DIEL

# every compiled build: (name, MATS, MEDIUM, instance file) -- 19 unfiltered, 7 filtered
TABLE = [
    ("render_kernel<LIGHT|DIFF>", LD, False, "pt_inst_light_diff.hip"),
    ("render_kernel<LIGHT|DIFF,medium>", LD, True, "pt_inst_light_diff.hip"),
    ("render_kernel<LIGHT|DIFF|COAT>", CO, False, "pt_inst_coat.hip"),
    ("render_kernel<LIGHT|DIFF|COAT; Beckmann>", CO | BECKMANN << DIST_SHIFT, False, "pt_inst_coat.hip"),
    ("render_kernel<LIGHT|DIFF|ROUGH_COND>", RC, False, "pt_inst_rough_cond.hip"),
    ("render_kernel<LIGHT|DIFF|ROUGH_COND; GGX>", RC | GGX << DIST_SHIFT, False, "pt_inst_rough_cond.hip"),
    ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL>", RD, False, "pt_inst_rough_diel.hip"),
    ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX>", RD | GGX << DIST_SHIFT, False, "pt_inst_rough_diel.hip"),
    ("render_kernel<generic>", 0, False, "pt_inst_generic.hip"),
    ("render_kernel<generic,medium>", 0, True, "pt_inst_generic.hip"),
    ("render_kernel<generic,sdf>", SDF, False, "pt_inst_sdf.hip"),
    ("render_kernel<generic,sdf,medium>", SDF, True, "pt_inst_sdf.hip"),
    ("render_kernel<generic,view>", VIEW, False, "pt_inst_view.hip"),
    ("render_kernel<generic,view,medium>", VIEW, True, "pt_inst_view.hip"),
    ("render_kernel<generic,sdf,view>", VIEW | SDF, False, "pt_inst_view_sdf.hip"),
    ("render_kernel<generic,sdf,view,medium>", VIEW | SDF, True, "pt_inst_view_sdf.hip"),
    ("render_kernel<generic,pick_random_light>", PICK, False, "pt_inst_pick.hip"),
    ("render_kernel<generic,pick_random_light,medium>", PICK, True, "pt_inst_pick.hip"),
    ("render_kernel<generic,env_importance_sampling>", ENVIS, False, "pt_inst_envis.hip"),
    ("render_kernel<LIGHT|DIFF,filter>", LD | FILTER, False, "pt_inst_filter_light_diff.hip"),
    ("render_kernel<LIGHT|DIFF,medium,filter>", LD | FILTER, True, "pt_inst_filter_light_diff.hip"),
    ("render_kernel<LIGHT|DIFF|COAT; Beckmann,filter>", CO | FILTER | BECKMANN << DIST_SHIFT, False, "pt_inst_filter_coat.hip"),
    ("render_kernel<LIGHT|DIFF|ROUGH_COND; GGX,filter>", RC | FILTER | GGX << DIST_SHIFT, False, "pt_inst_filter_rough_cond.hip"),
    ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX,filter>", RD | FILTER | GGX << DIST_SHIFT, False, "pt_inst_filter_rough_diel.hip"),
    ("render_kernel<generic,filter>", FILTER, False, "pt_inst_filter_generic.hip"),
    ("render_kernel<generic,medium,filter>", FILTER, True, "pt_inst_filter_generic.hip"),
]


# ---- the launcher, restated.  A scene is the dict of what launch_render read; every function returns (name, MATS, MEDIUM)
def _on_off(medium, mats, off, on):
    return (on, mats, True) if medium else (off, mats, False)


def launch_set_light_diff(medium, sc):
    return _on_off(medium, LD, "render_kernel<LIGHT|DIFF>", "render_kernel<LIGHT|DIFF,medium>")


def launch_set_generic(medium, sc):
    return _on_off(medium, 0, "render_kernel<generic>", "render_kernel<generic,medium>")


def launch_set_coat(medium, sc):
    if medium:
        return launch_set_generic(True, sc)
    if not sc["any_dist"] and sc["dist_mask"] == BECKMANN:
        return ("render_kernel<LIGHT|DIFF|COAT; Beckmann>", CO | BECKMANN << DIST_SHIFT, False)
    return ("render_kernel<LIGHT|DIFF|COAT>", CO, False)


def launch_set_rough_cond(medium, sc):
    if medium:
        return launch_set_generic(True, sc)
    if not sc["any_dist"] and sc["dist_mask"] == GGX:
        return ("render_kernel<LIGHT|DIFF|ROUGH_COND; GGX>", RC | GGX << DIST_SHIFT, False)
    return ("render_kernel<LIGHT|DIFF|ROUGH_COND>", RC, False)


def launch_set_rough_diel(medium, sc):
    if medium:
        return launch_set_generic(True, sc)
    if not sc["any_dist"] and sc["dist_mask"] == GGX:
        return ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX>", RD | GGX << DIST_SHIFT, False)
    return ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL>", RD, False)


def launch_set_sdf(medium, sc):
    return _on_off(medium, SDF, "render_kernel<generic,sdf>", "render_kernel<generic,sdf,medium>")


def launch_set_view(medium, sc):
    return _on_off(medium, VIEW, "render_kernel<generic,view>", "render_kernel<generic,view,medium>")


def launch_set_view_sdf(medium, sc):
    return _on_off(medium, VIEW | SDF, "render_kernel<generic,sdf,view>", "render_kernel<generic,sdf,view,medium>")


def launch_set_pick(medium, sc):
    return _on_off(medium, PICK, "render_kernel<generic,pick_random_light>", "render_kernel<generic,pick_random_light,medium>")


def launch_set_envis(medium, sc):
    return ("render_kernel<generic,env_importance_sampling>", ENVIS, False)          # whatever `medium` says


def launch_set_filter_generic(medium, sc):
    return _on_off(medium, FILTER, "render_kernel<generic,filter>", "render_kernel<generic,medium,filter>")


def launch_set_filter_light_diff(medium, sc):
    return _on_off(medium, LD | FILTER, "render_kernel<LIGHT|DIFF,filter>", "render_kernel<LIGHT|DIFF,medium,filter>")


def launch_set_filter_coat(medium, sc):
    if medium or sc["any_dist"] or sc["dist_mask"] != BECKMANN:
        return launch_set_filter_generic(medium, sc)
    return ("render_kernel<LIGHT|DIFF|COAT; Beckmann,filter>", CO | FILTER | BECKMANN << DIST_SHIFT, False)


def launch_set_filter_rough_cond(medium, sc):
    if medium or sc["any_dist"] or sc["dist_mask"] != GGX:
        return launch_set_filter_generic(medium, sc)
    return ("render_kernel<LIGHT|DIFF|ROUGH_COND; GGX,filter>", RC | FILTER | GGX << DIST_SHIFT, False)


def launch_set_filter_rough_diel(medium, sc):
    if medium or sc["any_dist"] or sc["dist_mask"] != GGX:
        return launch_set_filter_generic(medium, sc)
    return ("render_kernel<LIGHT|DIFF|DIEL|ROUGH_DIEL; GGX,filter>", RD | FILTER | GGX << DIST_SHIFT, False)


def launch_render(sc):
    am, medium = sc["active_mats"], sc["has_medium"] != 0
    if sc["filter_kind"] != 0:
        if not sc["generic"]:
            if am == LD:
                return launch_set_filter_light_diff(medium, sc)
            if am == CO:
                return launch_set_filter_coat(medium, sc)
            if am == RC:
                return launch_set_filter_rough_cond(medium, sc)
            if am == RD:
                return launch_set_filter_rough_diel(medium, sc)
        return launch_set_filter_generic(medium, sc)
    if sc["env_is"]:
        return launch_set_envis(medium, sc)
    if sc["pick_random_light"]:
        return launch_set_pick(medium, sc)
    if sc["view"]:
        return launch_set_view_sdf(medium, sc) if sc["n_sdfs"] else launch_set_view(medium, sc)
    if sc["n_sdfs"]:
        return launch_set_sdf(medium, sc)
    if not sc["generic"]:
        if am == LD:
            return launch_set_light_diff(medium, sc)
        if am == CO:
            return launch_set_coat(medium, sc)
        if am == RC:
            return launch_set_rough_cond(medium, sc)
        if am == RD:
            return launch_set_rough_diel(medium, sc)
    return launch_set_generic(medium, sc)


# ---- the input space
ACTIVE_MATS = [LD, CO, RC, RD,                                  # the four compiled masks
               CO | ROUGH_COND, RD | COAT, LD | COND,           # supersets of compiled masks (cornell_mixed's kind)
               LIGHT, LD | DIEL, LD | ROUGH_DIEL,               # subsets of compiled masks
               0]
AXES = [("active_mats", ACTIVE_MATS), ("has_medium", [0, 1]), ("n_sdfs", [0, 3]), ("view", [0, 1]), ("pick_random_light", [0, 1]),
        ("env_is", [0, 1]), ("dist_mask", list(range(8))),     # every subset of {Beckmann, Phong, GGX}
        ("filter_kind", [0, 1, 2, 3, 4]),                       # PRT_FILTER_NONE, box, tent, Gaussian, Blackman-Harris
        ("generic", [0, 1]), ("any_dist", [0, 1])]


def refused(sc):
    """the combinations no launch can have; nothing else is left out"""
    # pack_scene (prt_upload_scene): the light pick is not built together with SDF primitives or a debug view
    if sc["pick_random_light"] and (sc["n_sdfs"] or sc["view"]):
        return True
    # pack_scene: environment sampling is built for surfaces only (no global medium, SDF primitives, debug view, pick_random_light)
    if sc["env_is"] and (sc["has_medium"] or sc["n_sdfs"] or sc["view"] or sc["pick_random_light"]):
        return True
    # prt_set_pixel_filter: no filter instances for a debug view, SDF primitives (geom_flags, which a scene with SDF primitives must carry), the
    # light pick or environment sampling
    if sc["filter_kind"] and (sc["view"] or sc["n_sdfs"] or sc["pick_random_light"] or sc["env_is"]):
        return True
    return False


def scenes():
    names = [a[0] for a in AXES]
    for values in itertools.product(*[a[1] for a in AXES]):
        sc = dict(zip(names, values))
        if not refused(sc):
            yield sc


@pytest.fixture(scope="module")
def emu():
    import emu_api
    emu_api.lib()
    return emu_api


def test_the_restated_launcher_only_names_builds_of_the_table():
    """(of this file's own two statements: a typing error in either shows here, whatever the code under test does)"""
    rows = {(n, m, med) for n, m, med, _ in TABLE}
    assert len(TABLE) == 26 and len(rows) == 26 and len({(m, med) for _, m, med in rows}) == 26 and len({n for n, _, _ in rows}) == 26
    assert sum(1 for r in TABLE if r[1] & FILTER) == 7
    reached = {launch_render(sc) for sc in scenes()}
    assert reached == rows, (reached - rows, rows - reached)


def test_variant_table_is_the_compiled_builds(emu):
    """one row per (MATS, MEDIUM) pair with the name prt_kernel_variant reports and the instance file that compiles it: exactly the 26 builds,
    every instance file of the source tree named, and each file instantiating its own group of rows and nothing else"""
    table = emu.variant_table()
    assert sorted(table) == sorted((m, med, n, f) for n, m, med, f in TABLE), table
    hip = os.path.join(ROOT, "photorealistic-rendering-using-opencl_amd", "csrc", "hip")
    files = sorted(f for f in os.listdir(hip) if f.startswith("pt_inst_") and f.endswith(".hip"))
    assert files == sorted({f for _, _, _, f in TABLE}) and len(files) == 15
    for f in files:
        code = [l.strip() for l in open(os.path.join(hip, f)).read().split("\n") if l.strip() and not l.startswith("//")]
        group = f[len("pt_inst_"):-len(".hip")].upper()
        assert code == ['#include "pt_render.h"', "namespace prt { PT_VARIANTS_%s(PT_INSTANTIATE_VARIANT) }" % group], (f, code)


def test_select_variant_over_its_whole_input_space(emu):
    """every combination of the inputs that a launch can have (AXES minus refused()): the row select_variant returns is the build the restated
    launcher names -- name, MATS and MEDIUM --, it is a row of the table, and every row of the table is some combination's"""
    table = {(m, med, n) for m, med, n, _ in emu.variant_table()}
    reached, n, bad = set(), 0, []
    for sc in scenes():
        got = emu.select_variant(sc["active_mats"], sc["has_medium"], sc["n_sdfs"], sc["view"], sc["pick_random_light"], sc["env_is"], sc["dist_mask"],
                                 sc["filter_kind"], sc["generic"], sc["any_dist"])
        name, mats, medium = launch_render(sc)
        n += 1
        if got != (mats, medium, name) or got not in table:
            bad.append((sc, got, (mats, medium, name)))
        else:
            reached.add(got)
    # unfiltered: 2 x 2 x 2 of medium, SDFs and view, + the light pick x medium, + environment sampling = 11; filtered: 4 kinds x medium = 8; each
    # times 11 masks x 8 distribution masks x generic x any_dist
    assert n == (11 + 8) * len(ACTIVE_MATS) * 8 * 2 * 2 == 6688
    assert not bad, "%d of %d combinations; the first: %s" % (len(bad), n, bad[:3])
    assert reached == table, table - reached

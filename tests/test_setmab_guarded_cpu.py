"""CPU: every rc_setmab_* prototype of include/rechorus_hip.h is guarded (tests/setmab_guard_table.py GUARDED, with cases in
tests/test_gpu_setmab_guard_bands.py) or exempt with a reason, and each named engine wrapper exists and reaches its entry point --
what tests/test_listenc_guarded_cpu.py holds tests/listenc_guard_table.py to."""
import os
import re

from conftest import ROOT
import cfkg_guard_table as CT
import chorus_guard_table as CHT
import dcnv2_guard_table as DT
import guard_table as T
import listenc_guard_table as LT
import setmab_guard_table as MT
import slrc_guard_table as ST

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")


def header_setmab_entry_points():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(rc_setmab_\w+)\s*\(", text))


def test_every_setmab_prototype_is_guarded_or_exempt():
    declared = header_setmab_entry_points()
    assert declared == {"rc_setmab_check_shape", "rc_setmab_fwd", "rc_setmab_bwd", "rc_setmab_bwd_workspace_bytes"}
    both = sorted(set(MT.GUARDED) & set(MT.EXEMPT))
    assert not both, f"both guarded and exempt: {both}"
    missing = sorted(declared - set(MT.GUARDED) - set(MT.EXEMPT))
    assert not missing, f"rc_setmab_* entry points without a guard case or an exemption in tests/setmab_guard_table.py: {missing}"
    stale = sorted((set(MT.GUARDED) | set(MT.EXEMPT)) - declared)
    assert not stale, f"tests/setmab_guard_table.py names entry points the header does not declare: {stale}"
    for name, why in MT.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) >= 10 and "\n" not in why, name
    # no name overlaps with the other tables: one table per prototype
    mine = set(MT.GUARDED) | set(MT.EXEMPT)
    for other in (T, ST, CT, CHT, DT, LT):
        assert not mine & (set(other.GUARDED) | set(other.EXEMPT)), other.__name__


def test_the_status_returning_prototypes_are_spelled_as_the_enum():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in header_setmab_entry_points():
        m = re.search(r"([\w ]+?)\s+%s\s*\(" % re.escape(name), text)
        kind = " ".join(m.group(1).split()[-2:])
        assert kind.endswith("size_t") or kind == "enum rc_status", (name, kind)
        assert (name in MT.GUARDED) <= (kind == "enum rc_status"), name


def test_every_entry_point_cites_the_reference_lines_it_replaces():
    text = open(HEADER).read()
    section = text[text.index("set attention: one post-norm"):]
    assert "SetRank.py:29-56" in section[:section.index("rc_setmab_check_shape(")] and ":67-80" in section[:section.index("rc_setmab_check_shape(")]
    for name in ("rc_setmab_fwd", "rc_setmab_bwd"):
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "SetRank.py:29-56" in comment, name


def test_every_guarded_wrapper_exists_and_has_cases():
    from rechorus_amd import engine
    cases = open(os.path.join(ROOT, "tests", "test_gpu_setmab_guard_bands.py")).read()
    src = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    for name, entry in MT.GUARDED.items():
        assert callable(getattr(engine, entry["wrapper"], None)), (name, entry["wrapper"])
        assert entry["cases"], name
        assert entry.get("deterministic", True) is True          # no atomics: every result is compared bit for bit
        for fn in entry["cases"]:
            assert re.search(r"^def %s\(" % re.escape(fn), cases, flags=re.M), (name, fn)
        # the wrapper really reaches the entry point
        body = re.search(r"^def %s\(.*?(?=^def |^class |\Z)" % re.escape(entry["wrapper"]), src, flags=re.M | re.S).group(0)
        assert '"%s"' % name in body, name


def test_every_case_is_listed_in_the_table_and_every_listed_case_reaches_its_entry_point():
    import test_gpu_setmab_guard_bands as GB
    fns = {p.values[0] for p in GB.CASES} | {p.values[0] for p in GB.STACK_CASES} | {p.values[0] for p in GB.MODEL_CASES}
    by_name = {f.__name__: f for f in fns}
    assert len(GB.CASES) >= 8 and len({p.id for p in GB.CASES}) == len(GB.CASES) and len(GB.STACK_CASES) >= 2 and len(GB.MODEL_CASES) >= 2
    # the shared [nq, d] query source and a null pad are among the cases, beside per-list queries and a mask
    kinds = {p.values[1][-2:] for p in GB.CASES}
    assert kinds == {(1, 1), (1, 0), (0, 1), (0, 0)}
    for f in fns:
        for e in f.entries:
            if e in MT.GUARDED:
                assert f.__name__ in MT.GUARDED[e]["cases"], (f.__name__, e)
    for e, entry in MT.GUARDED.items():
        for name in entry["cases"]:
            assert name in by_name and e in by_name[name].entries, (e, name)

"""CPU: every rc_chorus_* prototype of include/rechorus_hip.h is guarded (tests/chorus_guard_table.py GUARDED, with cases in
tests/test_gpu_chorus_guard_bands.py) or exempt with a reason, and each named engine wrapper exists and reaches its entry point --
what tests/test_guarded_cpu.py holds tests/guard_table.py to for the `int rc_*(` prototypes."""
import os
import re

from conftest import ROOT
import chorus_guard_table as FT
import guard_table as T
import slrc_guard_table as ST
import cfkg_guard_table as CT

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")


def header_chorus_entry_points():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(rc_chorus_\w+)\s*\(", text))


def test_every_chorus_prototype_is_guarded_or_exempt():
    declared = header_chorus_entry_points()
    assert len(declared) == 9 and {"rc_chorus_check_shape", "rc_chorus_scores", "rc_chorus_fwd_bwd", "rc_chorus_scores_bwd",
                                   "rc_chorus_category_update_workspace_bytes", "rc_chorus_category_update"} <= declared
    both = sorted(set(FT.GUARDED) & set(FT.EXEMPT))
    assert not both, f"both guarded and exempt: {both}"
    missing = sorted(declared - set(FT.GUARDED) - set(FT.EXEMPT))
    assert not missing, f"rc_chorus_* entry points without a guard case or an exemption in tests/chorus_guard_table.py: {missing}"
    stale = sorted((set(FT.GUARDED) | set(FT.EXEMPT)) - declared)
    assert not stale, f"tests/chorus_guard_table.py names entry points the header does not declare: {stale}"
    for name, why in FT.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) >= 10 and "\n" not in why, name
    # the main table does not know them (its test would call them stale): one table per prototype
    assert not (set(FT.GUARDED) | set(FT.EXEMPT)) & (set(T.GUARDED) | set(T.EXEMPT))


def test_the_status_returning_prototypes_are_spelled_as_the_enum():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in header_chorus_entry_points():
        m = re.search(r"([\w ]+?)\s+%s\s*\(" % re.escape(name), text)
        kind = " ".join(m.group(1).split()[-2:])
        assert kind.endswith("size_t") or kind == "enum rc_status", (name, kind)
        assert (name in FT.GUARDED) <= (kind == "enum rc_status"), name


def test_every_guarded_wrapper_exists_and_has_cases():
    from rechorus_amd import engine
    cases = open(os.path.join(ROOT, "tests", "test_gpu_chorus_guard_bands.py")).read()
    src = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    for name, entry in FT.GUARDED.items():
        obj = engine
        for part in entry["wrapper"].split("."):
            assert hasattr(obj, part), (name, entry["wrapper"])
            obj = getattr(obj, part)
        assert callable(obj), (name, entry["wrapper"])
        assert entry["cases"], name
        assert entry.get("deterministic", True) is True          # no atomics: every Chorus result is compared bit for bit
        for fn in entry["cases"]:
            assert re.search(r"^def %s\(" % re.escape(fn), cases, flags=re.M), (name, fn)
        # the wrapper really reaches the entry point
        body = re.search(r"^def %s\(.*?(?=^def |^class |\Z)" % re.escape(entry["wrapper"]), src, flags=re.M | re.S).group(0)
        assert '"%s"' % name in body, name


def test_every_case_is_listed_in_the_table_and_every_listed_case_reaches_its_entry_point():
    import test_gpu_chorus_guard_bands as GB
    fns = {p.values[0] for p in GB.CASES}
    by_name = {f.__name__: f for f in fns}
    assert len(GB.CASES) >= 15 and len({p.id for p in GB.CASES}) == len(GB.CASES)
    for f in fns:
        for e in f.entries:
            assert e in FT.GUARDED or e in T.GUARDED or e in ST.GUARDED or e in CT.GUARDED, (f.__name__, e)
            if e in FT.GUARDED:
                assert f.__name__ in FT.GUARDED[e]["cases"], (f.__name__, e)
    for e, entry in FT.GUARDED.items():
        for name in entry["cases"]:
            assert name in by_name and e in by_name[name].entries, (e, name)

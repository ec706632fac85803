"""CPU: every rc_kda_* prototype of include/rechorus_hip.h is guarded (tests/kda_guard_table.py GUARDED, with cases in
tests/test_gpu_kda_guard_bands.py) or exempt with a reason, and each named engine wrapper exists and reaches its entry point --
what tests/test_din_guarded_cpu.py holds tests/din_guard_table.py to for the rc_din_* prototypes."""
import os
import re

from conftest import ROOT
import guard_table as T
import kda_guard_table as FT

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")


def header_kda_entry_points():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(rc_kda_\w+)\s*\(", text))


def test_every_kda_prototype_is_guarded_or_exempt():
    declared = header_kda_entry_points()
    assert declared == {"rc_kda_check_shape", "rc_kda_aggregate_fwd", "rc_kda_aggregate_bwd", "rc_kda_aggregate_bwd_workspace_bytes"}
    both = sorted(set(FT.GUARDED) & set(FT.EXEMPT))
    assert not both, f"both guarded and exempt: {both}"
    missing = sorted(declared - set(FT.GUARDED) - set(FT.EXEMPT))
    assert not missing, f"rc_kda_* entry points without a guard case or an exemption in tests/kda_guard_table.py: {missing}"
    stale = sorted((set(FT.GUARDED) | set(FT.EXEMPT)) - declared)
    assert not stale, f"tests/kda_guard_table.py names entry points the header does not declare: {stale}"
    for name, why in FT.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) >= 10 and "\n" not in why, name
    # the main table does not know them (its test would call them stale): one table per prototype
    assert not (set(FT.GUARDED) | set(FT.EXEMPT)) & (set(T.GUARDED) | set(T.EXEMPT))


def test_the_status_returning_prototypes_are_spelled_as_the_enum_and_cite_the_reference():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for name in header_kda_entry_points():
        m = re.search(r"([\w ]+?)\s+%s\s*\(" % re.escape(name), text)
        kind = " ".join(m.group(1).split()[-2:])
        assert kind.endswith("size_t") or kind == "enum rc_status", (name, kind)
        assert (name in FT.GUARDED) <= (kind == "enum rc_status"), name
    section = raw[raw.index("KDA relational dynamic aggregation"):]
    assert len(re.findall(r"KDA\.py:\d+", section)) >= 4       # the prototypes cite the reference lines they replace


def test_every_guarded_wrapper_exists_and_has_cases():
    from rechorus_amd import engine
    cases = open(os.path.join(ROOT, "tests", "test_gpu_kda_guard_bands.py")).read()
    src = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    for name, entry in FT.GUARDED.items():
        assert callable(getattr(engine, entry["wrapper"])), (name, entry["wrapper"])
        assert entry["cases"], name
        assert entry.get("deterministic", True) is True          # no atomics: every KDA result is compared bit for bit
        for fn in entry["cases"]:
            assert re.search(r"^def %s\(" % re.escape(fn), cases, flags=re.M), (name, fn)
        body = re.search(r"^def %s\(.*?(?=^def |^class |\Z)" % re.escape(entry["wrapper"]), src, flags=re.M | re.S).group(0)
        assert '"%s"' % name in body, name


def test_every_case_is_listed_in_the_table_and_every_listed_case_reaches_its_entry_point():
    import test_gpu_kda_guard_bands as GB
    fns = {p.values[0] for p in GB.CASES}
    by_name = {f.__name__: f for f in fns}
    assert len(GB.CASES) >= 10 and len({p.id for p in GB.CASES}) == len(GB.CASES)
    for f in fns:
        for e in f.entries:
            assert e in FT.GUARDED or e in T.GUARDED, (f.__name__, e)
            if e in FT.GUARDED:
                assert f.__name__ in FT.GUARDED[e]["cases"], (f.__name__, e)
    for e, entry in FT.GUARDED.items():
        for name in entry["cases"]:
            assert name in by_name and e in by_name[name].entries, (e, name)


def test_the_source_has_no_atomic():
    src = open(os.path.join(ROOT, "rechorus_amd", "csrc", "kda.hip")).read()
    code = re.sub(r"//[^\n]*", " ", src)
    assert not re.search(r"atomic", code, flags=re.I)

"""CPU: every rc_listenc_* prototype of include/rechorus_hip.h is guarded (tests/listenc_guard_table.py GUARDED, with cases in
tests/test_gpu_listenc_guard_bands.py) or exempt with a reason, and each named engine wrapper exists and reaches its entry point --
what tests/test_guarded_cpu.py holds tests/guard_table.py to for the `int rc_*(` prototypes."""
import os
import re

from conftest import ROOT
import cfkg_guard_table as CT
import chorus_guard_table as CHT
import dcnv2_guard_table as DT
import guard_table as T
import listenc_guard_table as LT
import slrc_guard_table as ST

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")


def header_listenc_entry_points():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(rc_listenc_\w+)\s*\(", text))


def test_every_listenc_prototype_is_guarded_or_exempt():
    declared = header_listenc_entry_points()
    assert declared == {"rc_listenc_check_shape", "rc_listenc_block_fwd", "rc_listenc_block_bwd", "rc_listenc_block_bwd_workspace_bytes"}
    both = sorted(set(LT.GUARDED) & set(LT.EXEMPT))
    assert not both, f"both guarded and exempt: {both}"
    missing = sorted(declared - set(LT.GUARDED) - set(LT.EXEMPT))
    assert not missing, f"rc_listenc_* entry points without a guard case or an exemption in tests/listenc_guard_table.py: {missing}"
    stale = sorted((set(LT.GUARDED) | set(LT.EXEMPT)) - declared)
    assert not stale, f"tests/listenc_guard_table.py names entry points the header does not declare: {stale}"
    for name, why in LT.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) >= 10 and "\n" not in why, name
    # no name overlaps with the other tables: one table per prototype
    mine = set(LT.GUARDED) | set(LT.EXEMPT)
    for other in (T, ST, CT, CHT, DT):
        assert not mine & (set(other.GUARDED) | set(other.EXEMPT)), other.__name__


def test_the_status_returning_prototypes_are_spelled_as_the_enum():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in header_listenc_entry_points():
        m = re.search(r"([\w ]+?)\s+%s\s*\(" % re.escape(name), text)
        kind = " ".join(m.group(1).split()[-2:])
        assert kind.endswith("size_t") or kind == "enum rc_status", (name, kind)
        assert (name in LT.GUARDED) <= (kind == "enum rc_status"), name


def test_every_entry_point_cites_the_reference_lines_it_replaces():
    text = open(HEADER).read()
    section = text[text.index("list encoder: one post-norm"):]
    for name in ("rc_listenc_block_fwd", "rc_listenc_block_bwd"):
        comment = section[:section.index(name + "(")].rsplit("/*", 1)[1]
        assert "PRM.py:64" in comment and "90-92" in comment, name


def test_every_guarded_wrapper_exists_and_has_cases():
    from rechorus_amd import engine
    cases = open(os.path.join(ROOT, "tests", "test_gpu_listenc_guard_bands.py")).read()
    src = open(os.path.join(ROOT, "rechorus_amd", "engine.py")).read()
    for name, entry in LT.GUARDED.items():
        assert callable(getattr(engine, entry["wrapper"], None)), (name, entry["wrapper"])
        assert entry["cases"], name
        assert entry.get("deterministic", True) is True          # no atomics: every result is compared bit for bit
        for fn in entry["cases"]:
            assert re.search(r"^def %s\(" % re.escape(fn), cases, flags=re.M), (name, fn)
        # the wrapper really reaches the entry point
        body = re.search(r"^def %s\(.*?(?=^def |^class |\Z)" % re.escape(entry["wrapper"]), src, flags=re.M | re.S).group(0)
        assert '"%s"' % name in body, name


def test_every_case_is_listed_in_the_table_and_every_listed_case_reaches_its_entry_point():
    import test_gpu_listenc_guard_bands as GB
    fns = {p.values[0] for p in GB.CASES} | {p.values[0] for p in GB.STACK_CASES} | {p.values[0] for p in GB.MODEL_CASES}
    by_name = {f.__name__: f for f in fns}
    assert len(GB.CASES) >= 8 and len({p.id for p in GB.CASES}) == len(GB.CASES) and len(GB.STACK_CASES) >= 2 and len(GB.MODEL_CASES) >= 2
    for f in fns:
        for e in f.entries:
            if e in LT.GUARDED:
                assert f.__name__ in LT.GUARDED[e]["cases"], (f.__name__, e)
    for e, entry in LT.GUARDED.items():
        for name in entry["cases"]:
            assert name in by_name and e in by_name[name].entries, (e, name)

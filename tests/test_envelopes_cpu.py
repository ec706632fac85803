"""CPU: every shape predicate the C ABI declares (rc_*_supported in include/rechorus_hip.h) has an entry in tests/envelopes.py, and
every test an entry names exists -- a new kernel envelope cannot land without a test at its edges.  The predicates themselves are not
called here: some query the device."""
import os
import re

from conftest import ROOT
import envelopes as E

HEADER = os.path.join(ROOT, "include", "rechorus_hip.h")
TESTS = os.path.join(ROOT, "tests")


def header_predicates():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(rc_\w+_supported)\s*\(", text))


def test_every_header_predicate_has_an_envelope_entry():
    declared = header_predicates()
    assert len(declared) >= 12, sorted(declared)
    missing = sorted(declared - set(E.ENVELOPES))
    assert not missing, f"shape predicates without an edge-case entry in tests/envelopes.py: {missing}"
    stale = sorted(set(E.ENVELOPES) - declared)
    assert not stale, f"tests/envelopes.py lists predicates the header no longer declares: {stale}"


def test_every_named_edge_test_exists():
    for name, entry in E.ENVELOPES.items():
        assert entry["edges"].strip() and entry["tests"], name
        for ref in entry["tests"]:
            fname, func = ref.split("::")
            path = os.path.join(TESTS, fname)
            assert os.path.isfile(path), (name, ref)
            assert re.search(r"^def %s\(" % re.escape(func), open(path).read(), flags=re.M), (name, ref)

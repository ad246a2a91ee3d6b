"""oracle/pin_kit -- the reference-side harness (golden_dump.rs), its case file and the comparator.

The Rust module cannot be compiled here; what runs on CPU: the case file is exactly what export_cases.py makes from the committed
golden vectors; a Python walk of the case file in golden_dump.rs's order of operations over the oracle's nodes reproduces every
expected vector and passes the comparator; the comparator notices a single flipped bit and a contradicting probe.  The check of the
module and the case file against the reference's own sources (tools/check_pin_kit.py) needs a checkout of the reference, which
this repository does not hold: it is run by hand, with DSPFX_REFERENCE naming that checkout."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIT = os.path.join(ROOT, "oracle", "pin_kit")


def _run(*args):
    return subprocess.run([sys.executable, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_cases_json_is_what_the_exporter_makes_from_the_committed_vectors(tmp_path):
    out = tmp_path / "cases.json"
    r = _run(os.path.join(KIT, "export_cases.py"), str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = json.load(open(out)), json.load(open(os.path.join(KIT, "cases.json")))
    assert a == b, "oracle/pin_kit/cases.json is stale: python oracle/pin_kit/export_cases.py"
    assert len(b["cases"]) >= 56 and {"fresh_reverb", "fresh_biquad", "chain_chain5_link3", "graph_fan_in_three", "dag_exact_7000"} <= {c["name"] for c in b["cases"]}


def test_emulated_harness_reproduces_every_vector_and_the_comparator_can_fail(tmp_path):
    out = tmp_path / "pin_out.json"
    r = _run(os.path.join(ROOT, "tools", "compare_pin.py"), "--emulate", str(out))
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run(os.path.join(ROOT, "tools", "compare_pin.py"), str(out))
    assert r.returncode == 0 and r.stdout.count("PASS") >= 56 and "FAIL" not in r.stdout and "EMULATED" in r.stdout, r.stdout + r.stderr
    d = json.load(open(out))
    d["results"][3]["y"][0][200] ^= 0x10                       # one sample, 16 ulp off
    bad = tmp_path / "bad.json"
    json.dump(d, open(bad, "w"))
    r = _run(os.path.join(ROOT, "tools", "compare_pin.py"), str(bad))
    assert r.returncode == 1 and r.stdout.count("FAIL") == 1, r.stdout
    d = json.load(open(out))
    d["probes"]["biquad_probe"]["y"][-1] ^= 1                  # DirectForm1::run rounds differently than the oracle assumes
    json.dump(d, open(bad, "w"))
    r = _run(os.path.join(ROOT, "tools", "compare_pin.py"), str(bad))
    assert r.returncode == 1 and "NONE of the candidate orders" in r.stdout, r.stdout

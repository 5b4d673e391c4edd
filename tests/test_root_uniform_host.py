"""CPU test of the root system's wave-uniform form (mpc_core.hpp::riccati_root_uniform: the partial-pivot exchanges as branches around row swaps, the ok / okp / finite flags
read once; what the shape-known wave kernel's sweeps call) against riccati_root_shape<true, 7>, the headline shape: a stand-alone host program
(tests/host_harness/root_uniform_host.cpp, its own main, g++ -ffp-contract=off) holds the two BIT FOR BIT in the return code, dd and nu[3] on inputs it makes itself --
tableaux that take every one of the 64 orders of exchanges, exact ties in the pivot compare at every compare, a zero, denormal, infinite and NaN pivot at each position,
inertia one too many and one too few, 10 000 well-scaled and 10 000 badly scaled systems (entries 1e-12 .. 1e11) -- and evaluates a boundary product of the partitioned
forward sweep with its products' factors in both orders.  The same program built with -fsanitize=address,undefined runs clean (executed directly; nothing sanitised is
loaded into Python)."""
import os
import re
import subprocess

import pytest

import _harness

FAMILIES = ("exchange_orders", "pivot_ties", "special_pivots", "inertia", "random_well_scaled", "random_badly_scaled", "boundary_product")


def _run(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


def _lines(out):
    rows = {}
    for m in re.finditer(r"^(\w+) cases=(\d+) mismatches=(\d+) codes=(\d+)/(\d+)/(\d+)(.*)$", out, re.M):
        rows[m.group(1)] = dict(cases=int(m.group(2)), bad=int(m.group(3)), codes=tuple(int(m.group(i)) for i in (4, 5, 6)), extra=m.group(7))
    return rows


@pytest.fixture(scope="module")
def report():
    out = os.path.join(_harness.BUILD, "root_uniform_host")
    r = _run(_harness._built(out, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", _harness.source("root_uniform_host"), "-o", out]))
    return r.returncode, r.stdout, _lines(r.stdout)


def test_uniform_root_equals_the_shape_known_root_bit_for_bit(report):
    rc, out, rows = report
    assert rc == 0 and "ALL EQUAL" in out
    assert set(rows) == set(FAMILIES)
    for name in FAMILIES:
        assert rows[name]["bad"] == 0 and rows[name]["cases"] > 0, name


def test_inputs_cover_what_they_are_made_for(report):
    _, _, rows = report
    assert "patterns=64" in rows["exchange_orders"]["extra"] and rows["exchange_orders"]["cases"] == 128      # every order of the six exchanges, with and without a counted pivot
    assert "tied_compares=0x3f" in rows["pivot_ties"]["extra"] and rows["pivot_ties"]["cases"] > 1000         # a tie at each of the six compares
    sp = rows["special_pivots"]
    assert sp["cases"] == 4 * 8 * 3 + 2 + 17 * 8 and sp["codes"][1] > 100 and sp["codes"][2] > 0              # breakdowns (0) and systems a special word leaves solvable
    inertia = rows["inertia"]
    assert inertia["cases"] == 10000 and inertia["codes"][0] >= 4 * 2000 - 50 and inertia["codes"][2] >= 1900  # one too many / too few: -1; the untouched system: 1
    assert rows["random_well_scaled"]["cases"] == 10000 and min(rows["random_well_scaled"]["codes"][0], rows["random_well_scaled"]["codes"][2]) > 1000
    assert rows["random_badly_scaled"]["cases"] == 10000 and all(c > 0 for c in rows["random_badly_scaled"]["codes"])
    assert rows["boundary_product"]["cases"] == 10000


def test_program_is_clean_under_address_and_undefined_sanitizers():
    r = _run(_harness.sanitized("root_uniform_host", []))
    assert r.returncode == 0 and "ALL EQUAL" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr

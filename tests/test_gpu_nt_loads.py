"""GPU: the staged ungrouped kernel (V_GLOBAL_S) with non-temporal column loads computes bit for bit what it computes with
default-policy loads (PRESTO_AMD_NT=0) and what the plain kernel computes (PRESTO_AMD_STAGED=0), at every level of the switch.

Q6 shape, PRESTO_AMD_STAGED=1 and PRESTO_AMD_NO_RANGES=1 as in tests/test_gpu_staged.py: one quad, a page short of a workgroup, a page
of several workgroups with rows behind its last quad, two pages of which the second is unaligned (scalar rows), and NULLs in the
later-stage columns.  The few-groups tier (Q1) keeps default-policy loads -- its source does not depend on the switch, which
tests/test_codegen_nt_loads.py pins -- so there is nothing of it to run here."""
import pytest

from tests.test_gpu_staged import bits, host_q6, q6_operator
from presto_amd.operators import to_pages

pytestmark = pytest.mark.gpu

LEVELS = ("1", "2")


def pages_of(oracle, case):
    if case == "two_pages_second_unaligned":
        host = host_q6(oracle, 0.1, 400001)
        return [host.get_region(0, 123457), host.get_region(123457, 400001 - 123457)]
    if case == "nulls_in_later_stages":
        return [host_q6(oracle, 0.1, 1 << 18, null_rate=0.1)]
    return [host_q6(oracle, 0.1, case)]


def run(monkeypatch, staged, nt, pages):
    monkeypatch.setenv("PRESTO_AMD_NO_RANGES", "1")
    monkeypatch.setenv("PRESTO_AMD_STAGED", staged)
    monkeypatch.setenv("PRESTO_AMD_NT", nt)
    op = q6_operator()
    out = to_pages(op, pages)
    name = op.kernelName()
    op.close()
    return bits([r for p in out for r in p.to_rows()]), name


@pytest.mark.parametrize("case", [4, 1023, (1 << 20) + 3, "two_pages_second_unaligned", "nulls_in_later_stages"])
def test_every_level_computes_what_level_0_and_the_plain_kernel_compute(gpu, oracle, monkeypatch, case):
    pages = pages_of(oracle, case)
    plain, plain_name = run(monkeypatch, "0", "0", pages)
    level0, name0 = run(monkeypatch, "1", "0", pages)
    assert "staged" in name0 and "staged" not in plain_name
    assert level0 == plain
    names = {name0}
    for level in LEVELS:
        got, name = run(monkeypatch, "1", level, pages)
        assert "staged" in name
        assert got == level0, (case, level)
        names.add(name)
    assert len(names) == 1 + len(LEVELS)   # (a kernel of its own per level)
    if isinstance(case, int) and case >= 1023:
        assert plain[1] > 0   # (rows pass the filter)

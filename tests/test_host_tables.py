"""The host-only scenario precompute (csrc/scenario_tables.h) under the address, leak and undefined-
behaviour sanitizers, without a GPU: tests/host_tables/host_tables_check.cpp builds, packs and
destroys one scenario per kernel family and feeds the two builders one faulty descriptor per error
message.  Every message of the header must show up in its output, so a new check needs a case."""
import os
import re

import host_program

REJECT = re.compile(r'reject\(err,\s*(MPCT_\w+),\s*"([^"]+)"\)')


def test_host_tables_under_sanitizers(tmp_path):
    stdout = host_program.run(host_program.build("host_tables_check", tmp_path))
    for name in ("shell3x3", "dtc 2x2:", "dtc 2x2, bounded", "mdband", "van de vusse nmpc"):
        assert "valid " + name in stdout, name
    # the dispatch key's Gram tables (gram_tables): built for the GPC and DTC scenarios, none for band and NMPC
    gram = {m.group(1): int(m.group(2)) for m in re.finditer(r"valid ([^:]+):.*gram (\d+) doubles", stdout)}
    assert gram["shell3x3 (derived CARIMA)"] == 30 * 5 * 3 * 272 and gram["dtc 2x2"] == 10 * 4 * 2 * 272, gram
    assert gram["mdband 2x(1+1)"] == 0 and gram["van de vusse nmpc"] == 0, gram

    header = open(os.path.join(host_program.CSRC, "scenario_tables.h")).read()
    checks = REJECT.findall(header)
    assert len(checks) >= 45, len(checks)  # the regex still finds the builders' error returns
    codes = {"MPCT_EINVAL": -1, "MPCT_ERANGE": -4}
    missing = [(c, m) for c, m in checks if 'rejected %d "%s"' % (codes[c], m) not in stdout]
    assert not missing, missing

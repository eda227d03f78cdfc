"""The prologue's pre-factored rows (csrc/scenario_tables.h qr_tables) on the host, without a GPU:
tests/host_tables/qr_tables_check.cpp under the address, leak and undefined-behaviour sanitizers.  The
program itself holds R_i'R_i = G_i'G_i and R_i'T_i = G_i'Phi_i (1e-13 of the matrices' norms), the
zeros left of each row's level, the cell index and the byte cap over every cell of Shell 3x3 and of a
2x2 plant with dead time; here its summary lines are checked for what the cases must have covered."""
import re

import host_program


def test_qr_tables_under_sanitizers(tmp_path):
    stdout = host_program.run(host_program.build("qr_tables_check", tmp_path))
    rows = {m.group(1): {k: float(v) for k, v in re.findall(r"(\w+)=(\S+)", m.group(2))}
            for m in re.finditer(r"^([^:\n]+): (qr_doubles=.*)$", stdout, flags=re.M)}
    assert set(rows) == {"shell3x3", "shell3x3 127x15", "deadtime 2x2"}, rows
    shell, dead = rows["shell3x3"], rows["deadtime 2x2"]
    # every cell Nu <= min(N2, 5) of N2 <= 30: 1.2 MB (nx = 35), under the cap; none for the VNS ranges
    assert shell["cells"] == sum(min(n2, 5) for n2 in range(1, 31)) == 140
    assert shell["qr_doubles"] == sum(3 * min(n2, 3 * nu) * (3 * nu + 35) for n2 in range(1, 31)
                                      for nu in range(1, min(n2, 5) + 1)) == 151440
    assert rows["shell3x3 127x15"]["qr_doubles"] == 0
    assert dead["cells"] == sum(min(n2, 4) for n2 in range(1, 13))
    for r in (shell, dead):
        assert r["short_cells"] > 0 and r["zero_columns"] > 0   # N2 < M and dead-time columns were met
        assert r["worst_rr"] <= 1e-13 and r["worst_rt"] <= 1e-13

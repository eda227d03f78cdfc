"""The host-only scenario precompute (csrc/scenario_tables.h) under the address, leak and undefined-
behaviour sanitizers, without a GPU: tests/host_tables/host_tables_check.cpp builds, packs and
destroys one scenario per kernel family and feeds the two builders one faulty descriptor per error
message.  Every message of the header must show up in its output, so a new check needs a case."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "model-predictive-control-tuning_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host_tables", "host_tables_check.cpp")
REJECT = re.compile(r'reject\(err,\s*(MPCT_\w+),\s*"([^"]+)"\)')


def test_host_tables_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_tables_check")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17",
                    "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, SRC, "-o", exe], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stderr.strip() == "", out.stderr[-4000:]  # no sanitizer report
    assert out.stdout.rstrip().endswith("ok")
    for name in ("shell3x3", "dtc 2x2:", "dtc 2x2, bounded", "mdband", "van de vusse nmpc"):
        assert "valid " + name in out.stdout, name

    header = open(os.path.join(CSRC, "scenario_tables.h")).read()
    checks = REJECT.findall(header)
    assert len(checks) >= 45, len(checks)  # the regex still finds the builders' error returns
    codes = {"MPCT_EINVAL": -1, "MPCT_ERANGE": -4}
    missing = [(c, m) for c, m in checks if 'rejected %d "%s"' % (codes[c], m) not in out.stdout]
    assert not missing, missing

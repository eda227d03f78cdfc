"""The staging layout of an ordered launch's cost records, without a GPU: csrc/mpct_dev.h xcd_row (the
XCD-major row of a workgroup slot, ragged last block included) and stage_row (the row of only the
requested fields, all 64 subsets) under the address, leak and undefined-behaviour sanitizers
(tests/host_tables/stage_rows_check.cpp).  The same rows on the device: tests/test_result_records_gpu.py."""
import host_program


def test_stage_rows_under_sanitizers(tmp_path):
    stdout = host_program.run(host_program.build("stage_rows_check", tmp_path))
    assert "xcd_row: injective and inside 8 * ceil(S / 8) rows for S = 1..2100" in stdout
    for my, nu in ((1, 1), (3, 3), (7, 5), (2, 3)):
        assert "stage_row: 64 subsets at my = %d, nu = %d" % (my, nu) in stdout
    assert "FAILED" not in stdout

"""The slot count of the metric launch's wide split, without a GPU: csrc/mpct_dev.h wide_slot_rule and
wide_slots under the address, leak and undefined-behaviour sanitizers
(tests/host_tables/wide_rule_check.cpp).  The split itself on the device: tests/test_wide_split_gpu.py."""
import host_program


def test_wide_slot_rule_under_sanitizers(tmp_path):
    stdout = host_program.run(host_program.build("wide_rule_check", tmp_path))
    assert "rule at S = 255, 256, 4096, 8192 on 256 CUs: 0 256 1024 0" in stdout
    assert "wide_slots: 0 without a permutation, 0 <= H <= S, forced counts kept" in stdout
    assert "FAILED" not in stdout

"""The per-Gaussian instance-run reduce (csrc/gsr_reduce.h) behind gsr_contribution_stats, gsr_backward_blend_abs and gsr_render_features_backward,
through the shipped package on the CPU: the SIMT build of the whole library behind the package's own loader, as in tests/test_contrib_cpu.py.  Frame,
checks and bars: tests/instance_run_frames.py -- runs of 144 instances, so the fold path and the skipped chunks run, which no other CPU test reaches.

Test infrastructure: the product never loads the SIMT library."""
import pytest

from test_simt_package_cpu import package_on_the_cpu, simt_lib  # noqa: F401  (fixture)
import instance_run_frames as F


def test_the_frame_has_whole_chunks_with_and_without_contributions():
    props = F.frame_properties()
    assert props["P"] == F.N_SMALL + 4


def test_contribution_stats(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        F.check_contribution_stats(pkg, "cpu", "instance_runs_cpu_contrib")


def test_absgrad(simt_lib):
    with package_on_the_cpu(simt_lib) as pkg:
        F.check_absgrad(pkg, "cpu", "instance_runs_cpu_absgrad")


@pytest.mark.parametrize("channels", F.FEATURE_CHANNELS)
def test_feature_gradient(simt_lib, channels):
    with package_on_the_cpu(simt_lib) as pkg:
        F.check_feature_gradient(pkg, "cpu", channels, f"instance_runs_cpu_features_c{channels}")

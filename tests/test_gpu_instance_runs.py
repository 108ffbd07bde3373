"""The per-Gaussian instance-run reduce (csrc/gsr_reduce.h) on the MI355X: the frame and the checks of tests/test_instance_runs_cpu.py on the device
(tests/instance_run_frames.py: runs of 144 instances -- the fold path, skipped chunks, the tail lanes of the last wave), each entry point against its
fp64 reference with that reference's bars, and two runs bit for bit."""
import pytest

import instance_run_frames as F

pytestmark = pytest.mark.gpu


def _pkg():
    import diff_gaussian_rasterization as pkg
    return pkg


def test_gpu_contribution_stats():
    F.check_contribution_stats(_pkg(), "cuda", "instance_runs_gpu_contrib")


def test_gpu_absgrad():
    F.check_absgrad(_pkg(), "cuda", "instance_runs_gpu_absgrad")


@pytest.mark.parametrize("channels", F.FEATURE_CHANNELS)
def test_gpu_feature_gradient(channels):
    F.check_feature_gradient(_pkg(), "cuda", channels, f"instance_runs_gpu_features_c{channels}")

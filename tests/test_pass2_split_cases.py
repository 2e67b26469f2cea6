"""CPU checks (oracle only) that the generated cases take the paths they are meant for: the
planted split ids of pass2_cases.py are small, in several pieces, not excluded and removed by
the reference's size filter in blocks that meet k_sf_plan's sparse conditions, and the mixed
batch of test_gpu_parity.py holds one block of either regrow plan."""
import pytest

from cases import mixed_regrow_blocks, mixed_regrow_plans
from pass2_cases import SPLIT_CASES, SF_SPARSE_MAX, assert_split_preconditions, split_case, split_figures


@pytest.mark.parametrize('name', sorted(SPLIT_CASES))
def test_split_case_preconditions(name):
    assert_split_preconditions(name)


def test_split_cases_cover_the_edges():
    """The walk's limits: a size filter of exactly kSfSparseMax with an id of 60-63 voxels, the
    same input one above it, and ids whose first piece alone would leave voxels behind."""
    assert split_case('big64_3d')[0]['size_filter'] == SF_SPARSE_MAX
    assert split_case('big65_3d')[0]['size_filter'] == SF_SPARSE_MAX + 1
    for name in ('big64_3d', 'big65_3d'):
        assert 60 <= split_figures(name)[0]['max_voxels'] <= 63
    for name in SPLIT_CASES:
        assert all(f['stale'] > 0 for f in split_figures(name)), name


@pytest.mark.parametrize('mode', ['2d', '3d'])
def test_mixed_regrow_plans(mode):
    config = dict({} if mode == '2d' else dict(apply_dt_2d=False, apply_ws_2d=False), sigma_seeds=1.0, size_filter=25)
    (sparse_a, nsmall_a), (sparse_b, _) = mixed_regrow_plans(config, mixed_regrow_blocks())
    assert sparse_a and nsmall_a > 0 and not sparse_b

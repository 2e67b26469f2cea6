"""bench.py's plain run and --dump-outputs: a plain run has every side leg off and --full turns
them on again (the --no-* options still take single legs out); dump_outputs writes the same
float64 files for the same step results, within its size bound; a measurement without the
single-stream stage pass still gives the pipeline figures."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = ('no_cpu_baseline', 'no_host', 'no_e2e', 'no_strong', 'no_threshcc', 'no_config5')


def test_plain_run_has_no_side_legs():
    a = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '3'])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert all(getattr(a, k) for k in LEGS)


def test_full_run_keeps_the_single_switches():
    a = bench.parse_args(['--full'])
    assert a.full and not any(getattr(a, k) for k in LEGS)
    a = bench.parse_args(['--full', '--no-e2e', '--dump-outputs', 'd'])
    assert a.no_e2e and a.dump_outputs == 'd'
    assert not any(getattr(a, k) for k in LEGS if k != 'no_e2e')


@pytest.mark.parametrize('argv', [['--steps', '0'], ['--warmup', '-1']])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def _step_results():
    """Two blocks as a step leaves them: one smaller than its sample share, one larger, ids with
    the block offset above 2^32 (exact in float64 only)."""
    order = []
    for bid, shape in ((3, (2, 4, 8)), (7, (8, 32, 32))):
        lab = torch.arange(int(np.prod(shape)), dtype=torch.int64).reshape(shape) % 97 + bid * (1 << 33)
        order.append(dict(output=lab, block_id=bid))
    return order, [(0, 96, 97), (0, 96, 97)], {'scan': np.array([0, 97]), 'n_ids': 194}


def test_dump_outputs_is_repeatable_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_VALUES', 1000)
    order, res, offsets = _step_results()
    dirs = [str(tmp_path / n) for n in ('a', 'b')]
    for d in dirs:
        bench.dump_outputs(d, 0, 1, order, res, offsets, torch.device('cpu'))
    assert sorted(os.listdir(dirs[0])) == ['block_results.npy', 'id_offsets.npy', 'labels_sample.npy']
    got = {n: np.load(os.path.join(dirs[0], n)) for n in os.listdir(dirs[0])}
    for n, a in got.items():
        assert a.dtype == np.float64
        assert np.array_equal(a, np.load(os.path.join(dirs[1], n))), n
    lab = got['labels_sample.npy']
    assert lab.shape == (2, 500) and lab.nbytes <= 8 * bench.DUMP_SAMPLE_VALUES
    # the small block whole (zero padded), the large one sampled from its own labels
    assert np.array_equal(lab[0, :64], order[0]['output'].reshape(-1).numpy().astype(np.float64))
    assert not lab[0, 64:].any()
    assert set(lab[1]) <= set(order[1]['output'].reshape(-1).numpy().astype(np.float64))
    assert lab[1].min() >= 7 * 2.0 ** 33
    assert np.array_equal(got['block_results.npy'], [[3, 0, 96, 97], [7, 0, 96, 97]])
    assert np.array_equal(got['id_offsets.npy'], [0, 97, 194])


def test_dump_outputs_of_ranks_share_the_bound(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE_VALUES', 1000)
    order, res, offsets = _step_results()
    for rank in range(2):
        bench.dump_outputs(str(tmp_path), rank, 2, order, res, offsets, torch.device('cpu'))
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ['%s_rank%d.npy' % (n, r) for n in ('block_results', 'id_offsets', 'labels_sample')
                     for r in range(2)]
    labs = [np.load(str(tmp_path / ('labels_sample_rank%d.npy' % r))) for r in range(2)]
    assert sum(a.nbytes for a in labs) <= 8 * 1000


def test_dump_size_bound_of_the_default_sample():
    # the label samples and, beside them, a few numbers per block: well inside 64 MB
    assert 8 * bench.DUMP_SAMPLE_VALUES + (1 << 20) <= 64 * 1000 * 1000


def test_roofline_without_stage_pass():
    m = dict(stage_1=None, dt=0.5, steps=5, outer_vox=1000, inner_vox=800, pass2_outer=0)
    rf = bench.roofline_of(bench.CONFIGS[3], m)
    assert rf['dom'] is None and rf['stage_gbs'] is None
    assert rf['ms_per_step'] == pytest.approx(100.0)
    assert rf['pipe'] == pytest.approx(bench.alg_bytes(bench.CONFIGS[3], 1000, 800, 0) / 0.1 / 1e9)

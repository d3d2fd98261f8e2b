"""CPU: the two host-side pieces every trainer's sample metrics share -- `common.fid.draw_until` (the draw loop of
sample_moments, sample_features and sample_swd) and `trainer.SampleMetrics` refusing a per-class score without labels."""
import numpy as np
import pytest


class CountingDraw:
    """draw() -> 100 rows, rows numbered across calls"""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return np.arange(100 * (self.calls - 1), 100 * self.calls)


@pytest.mark.parametrize("n,lengths", [(250, [100, 100, 50]), (200, [100, 100]), (1, [1])])
def test_draw_until_trims_the_last_batch_and_never_draws_again(n, lengths):
    from gan_lib_tensorflow_amd.common.fid import draw_until
    draw = CountingDraw()
    batches = list(draw_until(draw, n))
    assert [len(b) for b in batches] == lengths
    assert draw.calls == len(lengths)                      # an extra call would advance the device RNG
    assert np.array_equal(np.concatenate(batches), np.arange(n))


def test_draw_until_draws_lazily():
    from gan_lib_tensorflow_amd.common.fid import draw_until
    draw = CountingDraw()
    batches = draw_until(draw, 250)
    assert draw.calls == 0
    next(batches)
    assert draw.calls == 1


def test_msssim_diversity_without_labels_raises():
    from gan_lib_tensorflow_amd.trainer import SampleMetrics

    class Unlabelled(SampleMetrics):
        def _metric_batch(self, b):
            return np.zeros((b, 32, 32, 3), dtype=np.uint8), None

    with pytest.raises(TypeError, match="no labels"):
        Unlabelled().msssim_diversity(n_pairs=2)

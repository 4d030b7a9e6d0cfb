"""GPU: KFAC.update()'s queue -- launch sizes doubling from launch_first, defer_batches /
defer_bytes caps, merge groups by operand alignment, the short batch as x.last_rows,
merge_launches onto slab ranges, fast-path templates across reset(), the double-buffered packed
state -- over the schedules of tests/update_schedule_cases.py.  Every factor of every pass is
bitwise the exact reference sum_b X~_b^T X~_b / rows_b (test_update_schedules_host.py proves every
partial sum exact in fp32) and exactly symmetric."""
import numpy as np
import pytest

import update_schedule_cases as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("s", S.SCHEDULES, ids=S.IDS)
def test_schedule_exact(hip_device, s):
    def compare(what, got, want):
        g = got.cpu().numpy().astype(np.float64)
        if not np.array_equal(g, want):
            pytest.fail(f"{what}: {S.first_wrong(g, want)}")
        assert np.array_equal(g, g.T), f"{what}: not symmetric"

    S.run(s, hip_device, compare)

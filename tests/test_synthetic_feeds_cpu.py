"""The seeded stand-in datasets (synthetic_resident_dataset, synthetic_track_dataset, synthetic_subject_dataset) against
tests/golden/synthetic_feeds.npz, recorded by tests/golden/make_synthetic_feeds_golden.py before the two Gwilliams2022 builders were
folded into one: every value comes from one seeded generator, and the order of its draws decides all of them.  No GPU: the device
kernel and the WindowBank are recorders (tests/synthetic_feed_cases.py).

Exact: the recordings and the subject feed's X (draws and elementwise operations only), rec_subject, rec_task, onsets, seg_task,
seg_in_task, the window starts handed to add_track, both halves of the split, what ResidentSegments was constructed with, and the
first 8 values of feed.rng.randint(0, 1000, 8).  Within the case's stored tolerance 4 * n * 2^-24 * A (derived in the generator
script's docstring; a matrix product or a mean lies behind each element, and another host CPU may sum in another order): the
resident Y, the tracks, the subject feed's Y.  The stored values, as the script printed them:
    resident_short_last_task 5.3150e-06    resident_three_recordings 8.2676e-06    tracks_default_hop 4.5071e-06
    tracks_hop_3 4.8530e-06                tracks_empty_task 3.9671e-06            subject 5.9313e-06
A wrong or missing draw moves elements by O(1)."""
import os

import numpy as np
import pytest

from tests import synthetic_feed_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_feeds.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(K.CASES))
def test_builder_gives_the_recorded_dataset(name, golden, monkeypatch):
    K.patch_recorders(monkeypatch.setattr)
    got = K.run_case(name)
    want = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    tol = float(want.pop("tol"))
    assert 0.0 < tol < 1e-5 and set(got) == set(want)
    for key, w in want.items():
        g = np.asarray(got[key])
        assert g.shape == w.shape and g.dtype == w.dtype, key
        if key in K.TOLERANT:
            worst = float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max())
            print(f"{name}/{key}: largest difference {worst:.3e} (tolerance {tol:.3e})")
            assert worst <= tol, (key, worst, tol)
        else:
            assert np.array_equal(g, w), key


def test_cases_cover_what_they_claim(golden):
    """A short last task, three recordings per task, a hop other than T // 2, and a task without a segment whose track (and its
    draw) is skipped."""
    counts = lambda name: np.bincount(golden[name + "/seg_task"]).tolist()      # noqa: E731
    assert counts("resident_short_last_task") == [4, 4, 2] and len(golden["resident_short_last_task/recordings"]) == 6
    assert len(golden["resident_three_recordings/recordings"]) == 9
    assert np.diff(golden["tracks_default_hop/onsets"][0]).tolist() == [4, 4, 4]
    assert np.diff(golden["tracks_hop_3/onsets"][0]).tolist() == [3, 3, 3]
    assert golden["tracks_default_hop/starts_per_track"].tolist() == [4, 4, 2]
    assert counts("tracks_empty_task") == [1, 1, 1] and len(golden["tracks_empty_task/recordings"]) == 8
    assert len(golden["tracks_empty_task/tracks"]) == 3 and golden["tracks_empty_task/starts_per_track"].tolist() == [1, 1, 1]
    assert golden["subject/X"].shape == (K.S, K.C, 67) and golden["subject/Y"].shape == (K.F, 67)

"""``krylov_amd._loop.stop_rule_loop``, the one outer loop of every driver,
on a scripted device: ``run`` hands out a fixed list of rows chunk by chunk
and, as the device does, ends a chunk after the first row that meets the
criterion. Every expected history is written out by hand.
"""
import numpy as np
import pytest

from krylov_amd._loop import stop_rule_loop


class Script:
    """A device that produces ``rows`` in order; ``mid_after``: a mid-step row
    handed out once that many rows are out (bicgstab's mid-step stop)."""

    def __init__(self, rows, criterion, mid_after=None, mid=None):
        self.rows, self.criterion = [np.asarray(r, dtype=float) for r in rows], criterion
        self.mid_after, self.mid = mid_after, mid
        self.calls = []  # (k, steps) of every run call

    def run(self, k, steps):
        self.calls.append((k, steps))
        out = []
        while len(out) < steps and k + len(out) < len(self.rows):
            if self.mid_after == k + len(out):
                return out, np.asarray(self.mid, dtype=float)
            out.append(self.rows[k + len(out)])
            if np.all(out[-1] <= self.criterion):
                break
        return out, None


def _entry(row):
    return row[0]  # one column: the reference's 0-d entry of a 1-D b


def _rechecks(values):
    it = iter(values)
    return lambda: next(it)


def test_first_meets_the_rule_and_recheck_confirms():
    dev = Script([[9.0]], 1.0)
    success, k, res = stop_rule_loop(0.5, 1.0, 10, dev.run, chunk=4, entry=_entry, recheck=_rechecks([0.25]))
    assert (success, k, res) == (True, 0, [0.25])
    assert dev.calls == []


def test_failed_recheck_stays_in_the_history_and_the_loop_goes_on():
    # row 1 meets the rule on the recurrence, its explicit residual (3.0) does
    # not; row 3 meets it again and its explicit residual (0.75) does
    dev = Script([[5.0], [0.5], [2.0], [0.9], [0.1]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=4, entry=_entry, recheck=_rechecks([3.0, 0.75]))
    assert (success, k) == (True, 4)
    assert res == [8.0, 5.0, 3.0, 2.0, 0.75]
    assert dev.calls == [(0, 4), (2, 4)]


def test_without_recheck_the_rule_alone_ends_the_loop():
    dev = Script([[5.0], [0.5], [2.0]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=4, entry=_entry)
    assert (success, k, res) == (True, 2, [8.0, 5.0, 0.5])
    assert dev.calls == [(0, 4)]


def test_first_meets_the_rule_without_recheck():
    dev = Script([[9.0]], 1.0)
    assert stop_rule_loop(1.0, 1.0, 10, dev.run, chunk=4, entry=_entry) == (True, 0, [1.0])
    assert dev.calls == []


def test_maxiter_at_a_chunk_boundary():
    dev = Script([[7.0], [6.0], [5.0], [4.0], [3.0]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, 4, dev.run, chunk=2, entry=_entry, recheck=_rechecks([]))
    assert (success, k, res) == (False, 4, [8.0, 7.0, 6.0, 5.0, 4.0])
    assert dev.calls == [(0, 2), (2, 2)]


def test_maxiter_in_the_middle_of_a_chunk_clips_the_steps():
    dev = Script([[7.0], [6.0], [5.0], [4.0], [3.0]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, 3, dev.run, chunk=2, entry=_entry, recheck=_rechecks([]))
    assert (success, k, res) == (False, 3, [8.0, 7.0, 6.0, 5.0])
    assert dev.calls == [(0, 2), (2, 1)]


def test_the_last_allowed_step_may_still_succeed():
    # the rule is tested before k == maxiter (cg.py:156-166)
    dev = Script([[7.0], [0.5]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, 2, dev.run, chunk=2, entry=_entry, recheck=_rechecks([0.5]))
    assert (success, k, res) == (True, 2, [8.0, 7.0, 0.5])


def test_maxiter_zero():
    dev = Script([[7.0]], 1.0)
    assert stop_rule_loop(8.0, 1.0, 0, dev.run, chunk=2, entry=_entry, recheck=_rechecks([])) == (False, 0, [8.0])
    assert dev.calls == []
    # ... and the rule still comes first
    assert stop_rule_loop(0.5, 1.0, 0, dev.run, chunk=2, entry=_entry, recheck=_rechecks([0.5])) == (True, 0, [0.5])


def test_maxiter_none_asks_for_whole_chunks():
    dev = Script([[7.0], [6.0], [5.0], [4.0], [3.0], [2.0], [0.5]], 1.0)
    success, k, res = stop_rule_loop(8.0, 1.0, None, dev.run, chunk=3, entry=_entry)
    assert (success, k, res) == (True, 7, [8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 0.5])
    assert dev.calls == [(0, 3), (3, 3), (6, 3)]


def test_block_of_three_columns_waits_for_the_slowest():
    # device rows carry a padded 4th column that never enters the history
    crit = np.array([1.0, 1.0, 1.0])
    rows = [[0.5, 0.5, 4.0, 0.0], [0.4, 0.4, 2.0, 0.0], [0.3, 0.3, 1.0, 0.0], [0.2, 0.2, 0.1, 0.0]]
    dev = Script(rows, np.array([1.0, 1.0, 1.0, np.inf]))
    explicit = np.array([0.3, 0.3, 0.99])
    success, k, res = stop_rule_loop(np.array([3.0, 3.0, 9.0]), crit, 10, dev.run, chunk=8,
                                     entry=lambda row: row[:3].copy(), recheck=lambda: explicit)
    assert (success, k) == (True, 3)
    np.testing.assert_array_equal(np.array(res), [[3.0, 3.0, 9.0], [0.5, 0.5, 4.0], [0.4, 0.4, 2.0], [0.3, 0.3, 0.99]])
    assert dev.calls == [(0, 8)]


def test_zero_d_entries():
    dev = Script([[5.0], [0.5]], np.float64(1.0))
    success, k, res = stop_rule_loop(np.float64(8.0), np.float64(1.0), 10, dev.run, chunk=4,
                                     entry=lambda row: np.float64(row[0]), recheck=lambda: np.float32(0.5))
    assert (success, k) == (True, 2)
    assert res == [8.0, 5.0, 0.5] and all(np.ndim(r) == 0 for r in res)
    assert type(res[-1]) is np.float32  # the recheck's own value, untouched


def test_mid_row_after_two_full_rows():
    dev = Script([[7.0], [6.0], [5.0]], 1.0, mid_after=2, mid=[0.75])
    chunks = []
    success, k, res = stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=4, entry=_entry, recheck=_rechecks([]),
                                     on_chunk=lambda k, rn: chunks.append((k, rn)))
    assert (success, k, res) == (True, 2, [8.0, 7.0, 0.75])
    assert chunks == [] and dev.calls == [(0, 4)]


def test_mid_row_with_no_full_row():
    dev = Script([[7.0], [6.0], [5.0]], 1.0, mid_after=2, mid=[0.75])
    chunks, steps = [], []
    success, k, res = stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=2, entry=_entry, recheck=_rechecks([]),
                                     on_step=lambda k, rn: steps.append((k, rn)),
                                     on_chunk=lambda k, rn: chunks.append((k, rn)))
    assert (success, k, res) == (True, 2, [8.0, 7.0, 0.75])
    assert chunks == [(2, 6.0)] and steps == [(0, 7.0), (1, 6.0)]
    assert dev.calls == [(0, 2), (2, 2)]
    # at step 0 it replaces entry 0
    dev = Script([[7.0]], 1.0, mid_after=0, mid=[0.5])
    assert stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=2, entry=_entry, recheck=_rechecks([])) == (True, 0, [0.5])


def test_on_step_and_on_chunk():
    dev = Script([[7.0], [6.0], [5.0], [4.0], [0.5]], 1.0)
    steps, chunks = [], []
    success, k, res = stop_rule_loop(8.0, 1.0, 10, dev.run, chunk=2, entry=_entry, recheck=_rechecks([0.5]),
                                     on_step=lambda k, rn: steps.append((k, rn)),
                                     on_chunk=lambda k, rn: chunks.append((k, rn)))
    assert (success, k) == (True, 5)
    assert steps == [(0, 7.0), (1, 6.0), (2, 5.0), (3, 4.0), (4, 0.5)]
    assert chunks == [(2, 6.0), (4, 4.0), (5, 0.5)]


def test_empty_chunk_without_mid_raises():
    def run(k, steps):
        return [], None

    with pytest.raises(RuntimeError, match="no progress"):
        stop_rule_loop(8.0, 1.0, 10, run, chunk=4, entry=_entry, recheck=_rechecks([]))

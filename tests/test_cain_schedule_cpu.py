"""CPU: the non-timestep (recursive bisection) frame loop of the CAIN node, schedule.bisect_output_plan, against the reference's
generic_frame_loop(use_timestep=False) (tests/golden/cain_schedule_kat.json, tools/make_golden_cain.py) and the table of its output
positions and model calls."""
import json
import os
from fractions import Fraction

import pytest

from cfi_amd.schedule import InterpolationStateList, bisect_calls, bisect_output_plan


def positions(n_frames, multiplier, skip):
    states = InterpolationStateList(skip, True) if skip else None
    plan, tasks = bisect_output_plan(n_frames, multiplier, states)
    new = [pair + p for pair, outs, _ in tasks for p in outs]
    return [float(idx) if kind == "src" else float(new[idx]) for kind, idx in plan], sum(len(c) for _, _, c in tasks)


def test_plan_reproduces_the_reference_known_answers(golden_dir):
    with open(os.path.join(golden_dir, "cain_schedule_kat.json")) as f:
        kat = json.load(f)
    assert len(kat) >= 10
    for e in kat:
        got, calls = positions(e["n_frames"], e["multiplier"], e["skip"])
        assert got == e["positions"], e
        assert calls == e["model_calls"], e


@pytest.mark.parametrize("m,want,n_calls", [
    (2, ["1/2"], 1),
    (3, ["1/4", "3/4"], 3),
    (4, ["1/4", "1/2", "3/4"], 3),
    (5, ["1/8", "3/8", "5/8", "7/8"], 7),
    (7, ["1/8", "1/4", "3/8", "5/8", "3/4", "7/8"], 7),
    (10, [f"{k}/16" for k in (1, 3, 5, 7)] + ["1/2"] + [f"{k}/16" for k in (9, 11, 13, 15)], 15),
])
def test_output_positions_and_model_calls(m, want, n_calls):
    outs, calls = bisect_calls(m - 1)
    assert outs == [Fraction(s) for s in want]
    assert len(calls) == n_calls and len({p for p, _, _ in calls}) == n_calls      # one call per dyadic position
    seen = {Fraction(0), Fraction(1)}
    for pos, lo, hi in calls:        # every call reads frames that exist by then, and lands between them
        assert lo in seen and hi in seen and pos == (lo + hi) / 2
        seen.add(pos)


def test_list_entry_of_one_raises_up_front():
    with pytest.raises(ValueError, match="multiplier 1 of pair 1"):
        bisect_output_plan(4, [2, 1, 2])
    with pytest.raises(ValueError):
        bisect_output_plan(3, 1)
    with pytest.raises(ValueError):
        bisect_output_plan(3, [2, -1])
    # ... unless the pair is skipped (the list form consults the skip list with the pair's local index 0)
    plan, tasks = bisect_output_plan(3, [1, 1], InterpolationStateList([0], True))
    assert plan == [("src", 0), ("src", 1), ("src", 2)] and tasks == []


def test_zero_drops_the_pair_and_skipped_pairs_keep_their_frame():
    plan, tasks = bisect_output_plan(4, [3, 0, 2])
    assert plan == [("src", 0), ("new", 0), ("new", 1), ("src", 2), ("new", 2), ("src", 3)]
    assert [t[0] for t in tasks] == [0, 2]
    plan, tasks = bisect_output_plan(4, 3, InterpolationStateList([1], True))
    assert plan == [("src", 0), ("new", 0), ("new", 1), ("src", 1), ("src", 2), ("new", 2), ("new", 3), ("src", 3)]
    assert [t[0] for t in tasks] == [0, 2]

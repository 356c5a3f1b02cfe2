"""CPU: the bisection pair kind (cain.eval_pair) through the shared node loop (nodeloop.run_plan, its CPU branch) with a stand-in
engine over the torch restatement of the CAIN forward (tests/cain_restated.py), against the restated reference node loop — single
process and 2 ranks (gloo).  The frames must be equal."""
import os
import sys

import torch

import cain_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RestatedCain:
    """CainEngine.forward on the CPU: one restated model call per pair of the batch (test infrastructure only)."""

    def __init__(self, sd):
        self.sd, self.device = sd, torch.device("cpu")

    def forward(self, frames0, frames1):
        def nchw(f):
            return f.permute(2, 0, 1)[None].contiguous()

        with torch.no_grad():
            out = [cain_restated.cain_forward(self.sd, nchw(a), nchw(b)) for a, b in zip(frames0, frames1)]
        return torch.cat(out).permute(0, 2, 3, 1)


def _case():
    return cain_restated.seeded_state_dict(3), cain_restated.seeded_frames(4, 128, 128, 4, 21)      # RGBA clip: alpha is dropped


def _run(multiplier, skip):
    from cfi_amd.cain import eval_pair
    from cfi_amd.nodeloop import run_plan
    from cfi_amd.schedule import InterpolationStateList, bisect_output_plan

    sd, fr = _case()
    plan, tasks = bisect_output_plan(len(fr), multiplier, InterpolationStateList(skip, True) if skip else None)
    return run_plan(RestatedCain(sd), fr, plan, tasks, eval_pair, "CAIN VFI")


def test_bisection_pairs_through_the_loop():
    sd, fr = _case()
    for multiplier, skip in [(3, None), (4, [1])]:
        got = _run(multiplier, skip)
        want = cain_restated.node_frames(sd, fr, multiplier, skip)
        assert got.shape == want.shape and torch.equal(got, want), (multiplier, skip)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from pkgload import load_package

    load_package()
    import torch.distributed as dist

    from test_cain_loop_cpu import _run

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    out = _run(3, None)       # 3 pairs of 2 new frames: uneven shards
    if rank == 0:
        q.put(out.numpy())    # plain pickle: a torch tensor would travel through torch's shared-memory file descriptors
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_matches_one_process():
    from mp_util import run_ranks

    got = run_ranks(_worker, 2, timeout=300)
    sd, fr = _case()
    before = torch.get_num_threads()
    torch.set_num_threads(2)        # the ranks' thread count: the restated model's reductions then sum in the same order
    try:
        want = cain_restated.node_frames(sd, fr, 3)
    finally:
        torch.set_num_threads(before)
    assert got.shape == want.shape and torch.equal(got, want)

"""The frame loop of the pair-at-a-time nodes (FILM, M2M, IFRNet, GMFSS, IFUNet, CAIN, Sepconv, AMT, ATM, XVFI).  Of the eight
whole-network objects (netengine.py: FILM, M2M, CAIN, Sepconv, FLAVR, AMT, ATM, XVFI) all but FLAVR, whose forward takes a four-frame
window (flavr.py), run their clips here.

The reference walks the clip pair by pair (vfi_utils.generic_frame_loop, vfi_utils.py:149-389; film/__init__.py:63-113); the pairs are
independent, so the tasks are block-partitioned over ranks and the new frames all-gathered.  What differs between the
nodes is how one pair's new frames are computed — the ``pair_frames`` function each node passes in (film.film_pair, cain.eval_pair,
amt.pair_frames, atm.atm_pair, xvfi.xvfi_pair; m2m.run_plan binds m2m.timestep_pair); everything around it is here, once:

  * host side (hostpipe.py): every needed frame is uploaded once through pinned staging ahead of the compute streams; new frames and
    pass-through frames land in their final rows of the output tensor in the background;
  * pair lanes (lanes.py): pair j runs on lane j % n_lanes = its own engine on its own stream; the current (`main`) stream only carries
    the bookkeeping events: a frame's staging slot is released on `main` after `main` has waited for every lane that read it.
"""
import torch

from .dist import all_gather_frames, world
from .lanes import LaneSet, lanes_of, tell_lone_pair
from .schedule import shard_tasks


def run_plan(engine, frames, plan, tasks, pair_frames, name):
    """frames: [N,H,W,C] host tensor.  plan: ``("src", frame_idx)`` / ``("new", k)`` entries in output order; tasks: ``(pair_idx, new, ...)``
    tuples, ``new`` listing the pair's new frames, which are numbered k = 0.. in task order (schedule.generic_output_plan,
    bisect_output_plan, film_output_plan).  ``pair_frames(eng, f0, f1, task)`` runs one pair on the current stream and returns (or yields) its
    len(task[1]) new frames as [H,W,3] device tensors, in output order.  Returns the output as a [len(plan),H,W,3] host tensor."""
    if not plan:  # list multiplier of zeros: the reference fails in torch.cat of an empty list (vfi_utils.py:386)
        raise RuntimeError(f"{name}: every frame pair was dropped (multiplier 0 everywhere) - nothing to output")
    dev = engine.device
    frames = frames[..., :3]
    H, W = frames.shape[1:3]
    rank, ws = world()
    lo, hi = shard_tasks(tasks, rank, ws)
    counts = [sum(len(t[1]) for t in tasks[slice(*shard_tasks(tasks, r, ws))]) for r in range(ws)]
    mine = tasks[lo:hi]
    if dev.type != "cuda":  # stand-in engines of the CPU tests: same control flow without the device pipeline
        eng = engine.engines[0] if isinstance(engine, LaneSet) else engine

        def get(f):
            return frames[f].to(dev, torch.float32).contiguous()

        local = [x for t in mine for x in pair_frames(eng, get(t[0]), get(t[0] + 1), t)]
        local = torch.stack(local) if local else torch.empty((0, H, W, 3), dtype=torch.float32, device=dev)
        new = all_gather_frames(local, counts).cpu()
        src = frames.to("cpu", torch.float32)
        out = torch.empty((len(plan), H, W, 3), dtype=torch.float32)
        for i, (kind, idx) in enumerate(plan):
            out[i] = src[idx] if kind == "src" else new[idx]
        return out

    from .hostpipe import OutputWriter, Uploader, _stream
    main = torch.cuda.current_stream(dev)
    wr = OutputWriter(len(plan), H, W, dev)
    new_row = {}
    for i, (kind, idx) in enumerate(plan):
        if kind == "src":
            wr.put_host(i, frames[idx])
        else:
            new_row[idx] = i
    down = _stream(dev, "down")          # (the output writer's copy-back stream)
    if isinstance(engine, LaneSet):      # the lanes' streams stay clear of the copy streams' hardware queues where there are enough of them
        engine.apart_from = [down, _stream(dev, "up"), main]
    lane, n_lanes = lanes_of(engine, len(mine))
    tell_lone_pair(engine, n_lanes)      # an engine's own side-stream fork is for a lone pair
    order = sorted({f for t in mine for f in (t[0], t[0] + 1)})
    item_of = {f: i for i, f in enumerate(order)}
    up = Uploader(frames, order, dev, main, depth=min(max(4, n_lanes + 2), len(order))) if order else None
    k = 0                 # this rank's next new frame (one rank: its number in the plan)
    local = torch.empty((counts[rank], H, W, 3), dtype=torch.float32, device=dev) if ws > 1 else None   # gathered at the end
    pending = []          # completion events of lanes main has not waited for yet
    try:
        released = 0
        for j, task in enumerate(mine):
            pair = task[0]
            eng, st = lane(j % n_lanes)
            f0, f1 = up.get(item_of[pair], st), up.get(item_of[pair + 1], st)
            with torch.cuda.stream(st):      # (the pair's device tensors are allocated on its lane's stream)
                for x in pair_frames(eng, f0, f1, task):
                    if ws == 1:
                        wr.put_dev(new_row[k], x, st)
                        # x goes as soon as the loop lets it go, but the allocator hands its block out again only once the copy-back has
                        # read it.  (Holding x and polling put_dev's event instead cost 9-24 % on lanes: the polls stalled the launching thread.)
                        x.record_stream(down)
                    else:
                        local[k] = x
                    k += 1
                if n_lanes > 1:
                    done = torch.cuda.Event()
                    done.record(st)
                    pending.append(done)
            # Released only after the pair's LAST frame: some engines' prepare() keeps references to the ring-slot tensors and render()
            # re-reads them (IFRNet, IFUNet), so the `consumed` event must follow those reads.
            if released < item_of[pair + 1]:          # frames before pair+1 are never needed again (tasks ascend)
                for ev in pending:
                    main.wait_event(ev)
                pending = []
                while released < item_of[pair + 1]:
                    up.release(released)
                    released += 1
        for ev in pending:
            main.wait_event(ev)
        pending = []
        if ws > 1:
            new = all_gather_frames(local, counts)
            for n in range(new.shape[0]):
                wr.put_dev(new_row[n], new[n])
    finally:
        for ev in pending:      # (an error path: the staging rings go back with a `busy` event recorded on main)
            main.wait_event(ev)
        if up is not None:
            up.close()
    return wr.finish()

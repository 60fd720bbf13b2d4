"""The set-abstraction (SA) / feature-propagation (FP) OPERATOR stack of the RPN backbone, without the MLPs.

This is the unit BASELINE.json's metric is quoted on ("SA-stack points/sec per GPU, 16384-pt KITTI
scene"): per scene and level, furthest_point_sample -> gather_operation -> for each of the two MSG
scales ball_query -> grouping_operation(xyz) [-> grouping_operation(features)] -- i.e. 4 FPS +
4 gather + 8 ball_query + 14 grouping calls for the pyramid 16384 -> 4096 -> 1024 -> 256 -> 64
(reference call sequence: pointnet2_modules.py:39-59 + pointnet2_utils.py:249-255, shapes from
tools/cfgs/LI_Fusion_with_attention_use_ce_loss.yaml:56-64). The shared MLPs / max-pool between the
levels are stock PyTorch (out of scope), so the feature tensor entering each level is a synthetic
input of the right shape (C = 0 / 96 / 256 / 512).

Every buffer is allocated once; ``run()`` only launches kernels (through the extension stand-ins,
i.e. through the C ABI), so the sequence can be captured into a HIP graph (``capture()``).

The stack has two stages with very different machine behaviour:
  S  the sampling chain (scene index -> FPS -> gather, level after level): a strictly serial, latency-bound
     chain of one-workgroup-per-scene kernels that needs almost no LDS and no bandwidth;
  G  ball query + grouping of every level: wide, bandwidth-bound, depends on S only through the centres.
``pipelined=True`` runs S of batch k beside G of batch k-1 (double-buffered input clouds / centres / indices), so
that in steady state a step costs max(S, G) instead of S(level 1) + G. Consecutive steps consume DIFFERENT batches (the
reference's loop does: tools/train_rcnn.py:221-223, lib/net/train_functions.py): the input cloud has one resident buffer
per pipeline parity (``inputs[0 / 1]``); step k samples ``inputs[k & 1]`` and groups ``inputs[1 - (k & 1)]``, the batch of
step k-1, whose results are therefore complete once step k is (``SAStack.owners()`` says which buffer belongs to which
batch).
"""
import os

import torch

from . import pointnet2_cuda as ext

RPN_NPOINTS = (4096, 1024, 256, 64)
RPN_RADII = ((0.1, 0.5), (0.5, 1.0), (1.0, 2.0), (2.0, 4.0))
RPN_NSAMPLES = ((16, 32), (16, 32), (16, 32), (16, 32))
RPN_FEAT_CHANNELS = (0, 96, 256, 512)  # channels of the features grouped at each level
# FP modules, deepest first: (C of known feats, m known, n unknown), pointnet2_msg.py:232-235
RPN_FP = ((1024, 64, 256), (512, 256, 1024), (512, 1024, 4096), (256, 4096, 16384))


# the workloads bench.py times, by BASELINE.json config number: 2 = the RPN pyramid on 16384-point scenes (the metric's own
# configuration), 5 = one SA level on dense 65536-point scenes (centres = FPS 16384, r 0.5, nsample 64, grouping of the
# coordinates and of 64 feature channels: the ball-query / HBM stress case)
CONFIGS = {
    2: dict(n=16384, npoints=RPN_NPOINTS, radii=RPN_RADII, nsamples=RPN_NSAMPLES, feat_channels=RPN_FEAT_CHANNELS),
    5: dict(n=65536, npoints=(16384,), radii=((0.5,),), nsamples=((64,),), feat_channels=(64,)),
}


def sa_algorithmic_bytes(n=16384, npoints=RPN_NPOINTS, nsamples=RPN_NSAMPLES, feat_channels=RPN_FEAT_CHANNELS):
    """compulsory fp32/int32 traffic of one scene through the SA op stack (each input read once, each
    output written once), per kernel family -- SURVEY.md section 8(d)"""
    out = {"fps": 0, "gather": 0, "ball_query": 0, "group_xyz": 0, "group_feat": 0}
    cur = n
    for lvl, m in enumerate(npoints):
        out["fps"] += cur * 12 + m * 4
        out["gather"] += m * 4 + 3 * cur * 4 + 3 * m * 4
        for ns in nsamples[lvl]:
            out["ball_query"] += cur * 12 + m * 12 + m * ns * 4
            out["group_xyz"] += m * ns * 4 + 3 * cur * 4 + 3 * m * ns * 4
            c = feat_channels[lvl]
            if c:
                out["group_feat"] += m * ns * 4 + c * cur * 4 + c * m * ns * 4
        cur = m
    out["total"] = sum(out.values())
    return out


def fp_algorithmic_bytes(fp=RPN_FP):
    out = {"three_nn": 0, "three_interpolate": 0}
    for c, m, n in fp:
        out["three_nn"] += n * 12 + m * 12 + n * 24
        out["three_interpolate"] += c * m * 4 + n * 24 + c * n * 4
    out["total"] = sum(out.values())
    return out


class SAStack:
    def __init__(self, batch, n=16384, device="cuda", npoints=RPN_NPOINTS, radii=RPN_RADII, nsamples=RPN_NSAMPLES,
                 feat_channels=RPN_FEAT_CHANNELS, with_fp=False, fp=RPN_FP, seed=0, overlap=True, fused=True,
                 shared_index=True, pipelined=False, fused_sampling=False, queries_in_s=None, s_query_levels=None, stages=None):
        self.batch, self.n = batch, n
        # pipelined with THREE stages (stages=3; EPNET_SA_STAGES): the sampling chain is itself split in two -- S1, the level-1
        # sampling (2.1 of stage S's 3.1 ms: a latency-bound chain of one workgroup per scene), and S2, everything behind it
        # (levels 2-4, the ball queries, the FP neighbour searches: 17 short dispatches that wait for a place beside the wide kernels)
        # -- so that a step runs S1 of batch k beside S2 of batch k-1 beside G of batch k-2 from a ring of three buffer sets
        if stages is None:
            stages = int(os.environ.get("EPNET_SA_STAGES", "2"))
        self.stages = 3 if (pipelined and stages == 3 and fused_sampling and fused and shared_index) else (2 if pipelined else 1)
        self.ring = self.stages   # buffer sets (and resident input clouds) the schedule rotates through
        # overlap: FPS/gather of level l+1 depend only on the centres of level l (never on features), so
        # the sampling chain runs ahead on the launch stream while ball query + grouping of each level
        # follow on a second HIP stream
        self.overlap = overlap
        self.fused = fused                # grouped [xyz - centre ; features] from one kernel (epnet_group_concat)
        self.shared_index = shared_index  # one scene index per level for FPS + both ball queries
        self.pipelined = pipelined
        # epnet_sample_centres (FPS + row gather of the centres: 3 launches per level with the index build) instead of the
        # reference module's op-by-op sequence (transpose, fill, FPS, gather, transpose: 6 launches): 256-scene step 3.78 -> 3.66 ms
        self.fused_sampling = fused_sampling
        # Which ball queries run at the tail of stage S (behind the sampling -- and the neighbour search -- of the same batch, handing
        # their index tensors to the next step's grouping, double-buffered) instead of in front of their grouping in stage G:
        #  * with the FP ops in the step stage G carries 2.2 ms of interpolation on top of the groupings: all of them
        #    (256-scene step with FP ops: 7.17 (everything in G) -> 6.60 (three_nn in S) -> 6.2 ms);
        #  * without them, from ~240 scenes per step stage G (bandwidth-bound, grows with the batch) is the longer stage beside the
        #    latency-bound sampling chain: the queries of levels 2-4 go to stage S (256 scenes: 3.45 - 3.55 ms with every query in
        #    stage G -> 3.18 - 3.26 with level 2's in S -> 3.11 - 3.13 with levels 2-4, once the scene index build had become
        #    0.05 ms shorter; all levels: 3.52, level 1 alone: 3.49; at 128 scenes stage S is the longer one: 2.62 -> 2.69, so
        #    not there, and
        #    at 192 scenes 2.77 -> 2.88). Since the level-2 gather runs at the other levels' rate, level 2's queries are better off
        #    back in stage G, in front of that gather, where they run beside the level-1 sampling instead of in S's tail: levels
        #    3-4 only, below levels 2-4 in every one of 15 alternating rounds over three sessions, by 0.02 - 0.05 ms.
        # EPNET_SA_QUERIES_IN_S = 0: none, 1 (default): as above, 2: all levels; EPNET_SA_S_QUERY_LEVELS = "1,3": these (0-based)
        env_q = int(os.environ.get("EPNET_SA_QUERIES_IN_S", "1"))
        env_lv = os.environ.get("EPNET_SA_S_QUERY_LEVELS")
        every = frozenset(range(len(npoints)))
        if not pipelined:
            chosen = frozenset()
        elif s_query_levels is not None:
            chosen = frozenset(int(v) for v in s_query_levels)
        elif queries_in_s is not None:
            chosen = every if queries_in_s else frozenset()
        elif env_lv is not None:
            chosen = frozenset(int(v) for v in env_lv.split(",") if v.strip())
        elif self.stages == 3:
            chosen = every   # stage S2 has the room (and the grouping stage is the longest one)
        elif env_q == 2 or (env_q == 1 and with_fp):
            chosen = every
        elif env_q == 1 and batch * n >= 240 * 16384:
            chosen = every - {0, 1}
        else:
            chosen = frozenset()
        self.s_query_levels = chosen & every
        self.queries_in_s = self.s_query_levels == every
        # levels 2.. of the pyramid sample the centres of the level above: with the chain of tie-free round counts handed from level
        # to level (epnet_sample_centres_chain) their rounds are skipped wherever the answer is known to be 0 .. m-1
        self.chain = bool(int(os.environ.get("EPNET_SA_CHAIN", "1"))) and fused_sampling
        # the centre gather and the NEXT level's scene index: 1 (default) with the sampling in one call (epnet_sample_centres_chain_index:
        # the level-1 sampling workgroups do both in their epilogue, no dispatch behind the level-1 FPS); 2: the gather inside the next
        # level's index-build dispatch (epnet_scene_index_build_gathered, the default before the epilogue existed); 0: a gather and a
        # build of their own
        self.fuse_gather = int(os.environ.get("EPNET_SA_FUSE_GATHER", "1"))
        self._deferred = None
        self._next_built = None   # (level, parity) whose index the sampling call of the level above has built
        # the level-1 sampling issued ahead of stage G's first kernel (both wait for the level-1 index only): its one-per-CU workgroups
        # find their registers before the wide kernels fill the CUs. 128 scenes 2.62 -> 2.57 ms, 256 scenes with every query in
        # stage G 3.52 -> 3.43; nothing once stage G starts with an LDS-staged gather (queries of level 2 in stage S: 3.21 = 3.22)
        self.s_first = bool(int(os.environ.get("EPNET_SA_S_FIRST", "0" if self.s_query_levels else "1")))
        self.tail_scales = int(os.environ.get("EPNET_SA_TAIL_SCALES", "0"))
        self.multi_query = bool(int(os.environ.get("EPNET_SA_MULTI_QUERY", "1")))  # both scales of a level in one launch
        self.multi_group = bool(int(os.environ.get("EPNET_SA_MULTI_GROUP", "1")))  # both groupings of a level in one call
        self.ordered_query = bool(int(os.environ.get("EPNET_SA_ORDERED_QUERY", "1")))   # centres served in their spatial order (epnet_ball_query_ordered)
        self.side = None
        self.npoints, self.radii, self.nsamples, self.feat_channels = npoints, radii, nsamples, feat_channels
        self.with_fp, self.fp = with_fp, fp
        dev = torch.device(device)
        g = torch.Generator().manual_seed(seed)
        f32, i32 = torch.float32, torch.int32
        self.levels = []
        cur = n
        for lvl, m in enumerate(npoints):
            c = feat_channels[lvl]
            index_bytes = ext.scene_index_bytes(batch, cur) if shared_index else 0
            L = {
                "n": cur, "m": m, "c": c,
                # the flipped cloud of the unfused composition (pointnet2_modules.py:30): written by stage S, read by the grouping of
                # stage G one step later -- one per ring slot, like the centres
                "xyz_t_sets": [torch.empty((batch, 3, cur), dtype=f32, device=dev) for _ in range(self.ring if not fused else 1)],
                "temp": torch.empty((batch, cur), dtype=f32, device=dev),
                # (two stages: the sampling chain of one batch writes all levels in one go -- one tensor; three: S1 of batch k writes
                # level 1 while S2 of batch k-1 still reads its own)
                "fps_idx_sets": ([torch.empty((batch, m), dtype=i32, device=dev) for _ in range(3)] if self.stages == 3 else None),
                "fps_idx": None,
                "new_xyz_t": torch.empty((batch, 3, m), dtype=f32, device=dev),
                # what G reads from S, one set per pipeline parity
                "sets": [{"new_xyz": torch.empty((batch, m, 3), dtype=f32, device=dev),
                          "index": (torch.empty((index_bytes,), dtype=torch.uint8, device=dev) if index_bytes else None),
                          "prefix": torch.zeros((batch,), dtype=i32, device=dev),   # tie-free leading rounds of this level's sampling
                          # the last level's centres have no next level to index them: their own index for the ordered ball query
                          "centre_index": (torch.empty((ext.scene_index_bytes(batch, m),), dtype=torch.uint8, device=dev)
                                           if (shared_index and lvl + 1 == len(npoints) and ext.scene_index_bytes(batch, m)) else None)}
                         for _ in range(self.ring)],
                "features": (torch.randn((batch, c, cur), generator=g, dtype=f32).to(dev) if c else None),
                "scales": [],
            }
            for radius, ns in zip(radii[lvl], nsamples[lvl]):
                S = {"radius": radius, "ns": ns, "idx": torch.empty((batch, m, ns), dtype=i32, device=dev)}
                S["idx_sets"] = [S["idx"]] + ([torch.empty((batch, m, ns), dtype=i32, device=dev) for _ in range(self.ring - 1)]
                                              if lvl in self.s_query_levels else [])
                if fused:
                    S["grouped"] = torch.empty((batch, 3 + c, m, ns), dtype=f32, device=dev)
                    ws_bytes = ext.group_concat_workspace_bytes(batch, c, cur, m, ns)   # (long feature rows: a point-major copy)
                    S["workspace"] = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
                else:
                    S["grouped_xyz"] = torch.empty((batch, 3, m, ns), dtype=f32, device=dev)
                    S["grouped_feat"] = torch.empty((batch, c, m, ns), dtype=f32, device=dev) if c else None
                L["scales"].append(S)
            if L["fps_idx_sets"] is None:
                one = torch.empty((batch, m), dtype=i32, device=dev)
                L["fps_idx_sets"] = [one] * self.ring
            L["fps_idx"] = L["fps_idx_sets"][0]
            self.levels.append(L)
            cur = m
        self.fp_bufs = []
        if with_fp:
            for c, m, nn_ in fp:
                sets = [{"dist2": torch.empty((batch, nn_, 3), dtype=f32, device=dev),
                         "idx": torch.empty((batch, nn_, 3), dtype=i32, device=dev),
                         "weight": torch.empty((batch, nn_, 3), dtype=f32, device=dev)} for _ in range(self.ring)]
                self.fp_bufs.append({
                    "c": c, "m": m, "n": nn_,
                    "known_feats": torch.randn((batch, c, m), generator=g, dtype=f32).to(dev),
                    "sets": sets,                       # what the interpolation (stage G) reads from the neighbour search
                    "dist2": sets[0]["dist2"], "idx": sets[0]["idx"],   # (the last written set: see _search_fp)
                    "out": torch.empty((batch, c, nn_), dtype=f32, device=dev),
                })
        self.graphs = []
        self.replays = 0
        # the resident input clouds a captured graph reads: one per pipeline parity (one when every step stands alone)
        self.inputs = []
        self._prev_xyz = None   # eager pipelined steps: the cloud of the step before (stage G of the next step reads it)

    @property
    def static_xyz(self):
        """the input buffer of an unpipelined capture (a pipelined one has two: self.inputs)"""
        if self.pipelined and self.inputs:
            raise AttributeError("a pipelined stack has one input buffer per parity: use stack.inputs / stack.input_buffer()")
        return self.inputs[0] if self.inputs else None

    def input_buffer(self, step=None):
        """the resident cloud stage S of step `step` (default: the next one) reads -- the buffer a loader fills (stream-ordered
        behind the previous replay, whose stage G was the last reader of its old contents) instead of handing replay() a copy"""
        step = self.replays if step is None else step
        return self.inputs[step % len(self.inputs)]

    def owners(self):
        """After `replays` >= 1 steps of a pipelined stack: (parity sampled by the last step, parity it grouped). Buffers written
        by stage S (fps_idx, sets[p], the idx_sets[p] of the levels in s_query_levels, the FP search sets[p]) hold the batch
        of the LAST step; buffers written by stage G (grouped tensors, the single idx tensors of the other levels, the
        interpolation outputs) and the other parity's sets hold the batch of the step BEFORE it."""
        if self.stages == 3:
            raise RuntimeError("three stages: see owners3()")
        p = (self.replays - 1) & 1 if self.pipelined else 0
        return p, (1 - p if self.pipelined else 0)

    def owners3(self):
        """three stages, after `replays` >= 1 steps (the last one was step k = replays - 1): the buffer sets (slots of the ring) the
        last step's stages worked on -- (S1: level-1 sampling of batch k, S2: the rest of the sampling chain + queries + searches of
        batch k-1, G: groupings / interpolation of batch k-2). Slot S1 holds batch k's level-1 index, indices and prefix only (its
        other buffers still belong to batch k-3); slot S2 everything stage S writes; slot G that and, with the single-buffered
        outputs of stage G, the COMPLETE results of batch k-2."""
        k = self.replays - 1
        return k % 3, (k - 1) % 3, (k - 2) % 3

    def chain_identity_share(self, parity=None):
        """per level 2.. of the pyramid: the share of scenes whose sampling took the identity (the level above reported a tie-free
        prefix at least as long as this level's sample count) in the last step that sampled into set `parity`"""
        if not self.chain:
            return None
        if parity is None:
            parity = self.owners3()[1] if self.stages == 3 else self.owners()[0]
        out = []
        for lvl in range(1, len(self.levels)):
            known = self.levels[lvl - 1]["sets"][parity if self.pipelined else 0]["prefix"]
            out.append(round(float((known >= self.levels[lvl]["m"]).float().mean().item()), 4))
        return out

    # ---- stage S: the sampling chain of one level
    def _sample_level(self, L, cur_xyz, parity, index_built=False, defer_ok=False):
        """defer_ok (the pipelined schedule, where nobody reads a level's centres before the whole chain is through): the gather of
        this level's centres is left to the index build of the next level (epnet_scene_index_build_gathered: one dispatch for
        both) -- every dispatch on the chain waits for wave slots beside the wide kernels of stage G"""
        b, n, m = self.batch, L["n"], L["m"]
        P = L["sets"][parity]
        lvl = self.levels.index(L)
        pending, self._deferred = self._deferred, None
        built, self._next_built = self._next_built, None
        if pending is not None and pending[1:] == (lvl - 1, parity):   # cur_xyz has not been written yet: gather + index in one
            src_xyz, _, _ = pending
            prev = self.levels[lvl - 1]
            ext.scene_index_build_gathered_wrapper(b, prev["n"], n, src_xyz, prev["fps_idx_sets"][parity], cur_xyz, P["index"])
        elif built == (lvl, parity):   # by the sampling call of the level above, with cur_xyz
            pass
        elif P["index"] is not None and not index_built:
            ext.scene_index_build_wrapper(b, n, cur_xyz, P["index"])
        if self.fused_sampling:   # FPS + gather of the centres in one kernel (epnet_sample_centres)
            if not self.fused:
                L["xyz_t_sets"][parity].copy_(cur_xyz.transpose(1, 2))
            if self.chain:
                prefix_in = self.levels[lvl - 1]["sets"][parity]["prefix"] if lvl > 0 else None
                nxt = self.levels[lvl + 1]["m"] if lvl + 1 < len(self.levels) else 1
                nxt_L = self.levels[lvl + 1] if lvl + 1 < len(self.levels) else None
                defer = (defer_ok and self.fuse_gather and self.fused and nxt_L is not None
                         and nxt_L["sets"][parity]["index"] is not None and 1024 <= m <= 16384)
                if defer and self.fuse_gather == 1:
                    ext.sample_centres_index_wrapper(b, n, m, cur_xyz, P["index"], L["fps_idx_sets"][parity], P["new_xyz"],
                                                     nxt_L["sets"][parity]["index"], prefix_in, P["prefix"], nxt)
                    self._next_built = (lvl + 1, parity)
                else:
                    ext.sample_centres_wrapper(b, n, m, cur_xyz, P["index"], L["fps_idx_sets"][parity], None if defer else P["new_xyz"],
                                               prefix_in, P["prefix"], nxt)
                    if defer:
                        self._deferred = (cur_xyz, lvl, parity)
            else:
                ext.sample_centres_wrapper(b, n, m, cur_xyz, P["index"], L["fps_idx_sets"][parity], P["new_xyz"])
        else:                     # the reference module's sequence, op by op
            L["xyz_t_sets"][parity if not self.fused else 0].copy_(cur_xyz.transpose(1, 2))            # pointnet2_modules.py:30
            L["temp"].fill_(1e10)                                # pointnet2_utils.py:26
            if P["index"] is not None:
                ext.furthest_point_sampling_indexed_wrapper(b, n, m, cur_xyz, P["index"], L["temp"], L["fps_idx_sets"][parity])
            else:
                ext.furthest_point_sampling_wrapper(b, n, m, cur_xyz, L["temp"], L["fps_idx_sets"][parity])
            ext.gather_points_wrapper(b, 3, n, m, L["xyz_t_sets"][parity if not self.fused else 0], L["fps_idx_sets"][parity], L["new_xyz_t"])
            P["new_xyz"].copy_(L["new_xyz_t"].transpose(1, 2))    # pointnet2_modules.py:42-45
        return P["new_xyz"]

    def _idx(self, S, parity):
        """the neighbour-index tensor of a scale: one per pipeline parity when the queries run in stage S"""
        return S["idx_sets"][parity] if len(S["idx_sets"]) > 1 else S["idx"]

    # ---- stage G: neighbour search + grouping of one level
    def _query_scale(self, L, S, cur_xyz, parity):
        b, n, m = self.batch, L["n"], L["m"]
        P = L["sets"][parity]
        if P["index"] is not None:
            ext.ball_query_indexed_wrapper(b, n, m, S["radius"], S["ns"], P["new_xyz"], cur_xyz, P["index"], self._idx(S, parity))
        else:
            ext.ball_query_wrapper(b, n, m, S["radius"], S["ns"], P["new_xyz"], cur_xyz, self._idx(S, parity))

    def _group_scale(self, L, S, cur_xyz, parity):
        b, n, m = self.batch, L["n"], L["m"]
        if self.fused:   # pointnet2_utils.py:249-257 in one call
            ext.group_concat_wrapper(b, L["c"], n, m, S["ns"], cur_xyz, L["sets"][parity]["new_xyz"], L["features"],
                                     self._idx(S, parity), S["grouped"], True, S.get("workspace"))
        else:
            ext.group_points_wrapper(b, 3, n, m, S["ns"], L["xyz_t_sets"][parity], self._idx(S, parity), S["grouped_xyz"])
            if L["c"]:
                ext.group_points_wrapper(b, L["c"], n, m, S["ns"], L["features"], self._idx(S, parity), S["grouped_feat"])

    def _query_level(self, L, cur_xyz, parity):
        """the ball queries of all scales of the level: one launch over the shared index"""
        P = L["sets"][parity]
        # (the order pays from 32768 points up only -- epnet_ball_query_ordered itself ignores it below: no index is built for it there)
        centre_index = (self._centre_index(L, parity)
                        if (self.ordered_query and L["n"] > 16384 and P["index"] is not None and len(L["scales"]) <= 2) else None)
        if centre_index is not None:   # the centres in the order of their own scene index
            ext.ball_query_ordered_wrapper(self.batch, L["n"], L["m"], [S["radius"] for S in L["scales"]],
                                         [S["ns"] for S in L["scales"]], P["new_xyz"], cur_xyz, P["index"], centre_index,
                                         [self._idx(S, parity) for S in L["scales"]])
        elif P["index"] is not None and self.multi_query:
            ext.ball_query_multi_wrapper(self.batch, L["n"], L["m"], [S["radius"] for S in L["scales"]],
                                         [S["ns"] for S in L["scales"]], P["new_xyz"], cur_xyz, P["index"],
                                         [self._idx(S, parity) for S in L["scales"]])
        else:
            for S in L["scales"]:
                self._query_scale(L, S, cur_xyz, parity)

    def _centre_index(self, L, parity):
        """the scene index of this level's centres: the next level's index of its input (built by the sampling chain before anybody
        queries), or -- last level with >= 1024 centres -- one built here, just before the query that reads it"""
        lvl = self.levels.index(L)
        if lvl + 1 < len(self.levels):
            return self.levels[lvl + 1]["sets"][parity]["index"] if self.shared_index else None
        own = L["sets"][parity].get("centre_index")
        if own is not None:
            ext.scene_index_build_wrapper(self.batch, L["m"], L["sets"][parity]["new_xyz"], own)
        return own

    def _group_scales(self, L, cur_xyz, parity):
        """the groupings of all scales of the level: one call (feature rows staged once for both scales)"""
        if self.fused and self.multi_group and len(L["scales"]) > 1:
            ext.group_concat_multi_wrapper(self.batch, L["c"], L["n"], L["m"], [S["ns"] for S in L["scales"]], cur_xyz,
                                           L["sets"][parity]["new_xyz"], L["features"], [self._idx(S, parity) for S in L["scales"]],
                                           [S["grouped"] for S in L["scales"]], True)
        else:
            for S in L["scales"]:
                self._group_scale(L, S, cur_xyz, parity)

    def _group_level(self, L, cur_xyz, parity):
        self._query_level(L, cur_xyz, parity)
        self._group_scales(L, cur_xyz, parity)

    def _side_stream(self, device):
        if self.side is None:
            self.side = torch.cuda.Stream(device=device)
        return self.side

    def run(self, xyz):
        """xyz (B,N,3) contiguous fp32 on the stack's device; all outputs land in self.levels"""
        main = torch.cuda.current_stream(xyz.device)
        side = self._side_stream(xyz.device) if self.overlap else None
        cur_xyz = xyz
        built = False
        for lvl, L in enumerate(self.levels):
            new_xyz = self._sample_level(L, cur_xyz, 0, index_built=built)
            built = False
            nxt = self.levels[lvl + 1] if lvl + 1 < len(self.levels) else None
            if self.ordered_query and L["n"] > 16384 and nxt is not None and nxt["sets"][0]["index"] is not None:
                # the ordered ball query of this level walks the index of its centres = the next level's index of its input
                ext.scene_index_build_wrapper(self.batch, L["m"], new_xyz, nxt["sets"][0]["index"])
                built = True
            if side is not None:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._group_level(L, cur_xyz, 0)
            else:
                self._group_level(L, cur_xyz, 0)
            cur_xyz = new_xyz
        if side is not None:
            main.wait_stream(side)
        if self.with_fp:
            self._run_fp(xyz, 0)

    def run_pipelined(self, xyz, prev_xyz, step):
        """one steady-state step: stage S of this batch (into set `step & 1`) beside stage G of the previous
        batch (`prev_xyz`, whose stage S filled the other set in the step before). Measured dead ends: splitting
        stage G further (ball queries beside groupings on a third stream) gains nothing eagerly and loses under a
        graph; building the next batch's level-1 index one step early (three rotating buffers) only moves the
        contention, the step stays stage-G bound."""
        parity = step & 1
        main = torch.cuda.current_stream(xyz.device)
        side = self._side_stream(xyz.device)
        first = self.levels[0]
        if first["sets"][parity]["index"] is not None:
            # built before stage G is issued: a one-workgroup-per-scene kernel with 64 KB of LDS cannot find a free
            # CU once the wide stage-G kernels are in flight
            ext.scene_index_build_wrapper(self.batch, first["n"], xyz, first["sets"][parity]["index"])
        forked = torch.cuda.Event()
        forked.record(main)
        s_cur = xyz
        if self.s_first:   # the level-1 sampling is issued before the first kernel of stage G (which depends on the index build only)
            s_cur = self._sample_level(first, xyz, parity, index_built=True, defer_ok=True)
        side.wait_event(forked)
        with torch.cuda.stream(side):
            # order inside stage G: everything of the previous batch's stage S is complete, so only "ball query
            # before its grouping" binds. The level-1 FPS of stage S holds ~80 % of every CU's vector registers
            # for the first 2.5 ms of the step: the LDS-staged feature gathers of levels 2-4 (few registers) run
            # beside it, the level-1 ball queries (occupancy-hungry) after it.
            inputs = [prev_xyz] + [L["sets"][1 - parity]["new_xyz"] for L in self.levels[:-1]]
            # (the index tensors of the levels in s_query_levels are ready: their part of stage G is the groupings alone)
            in_s = self.s_query_levels
            deep = list(enumerate(zip(self.levels, inputs)))[1:]
            for lvl, (L, cur) in deep[:1]:   # level 2 (indexed queries: few registers) then its gathers beside the level-1 FPS
                if lvl not in in_s:
                    self._query_level(L, cur, 1 - parity)
                self._group_scales(L, cur, 1 - parity)
            for lvl, (L, cur) in deep[1:]:
                if lvl not in in_s:
                    self._query_level(L, cur, 1 - parity)
            for lvl, (L, cur) in deep[1:]:
                self._group_scales(L, cur, 1 - parity)
            if 0 in in_s:
                self._group_scales(first, prev_xyz, 1 - parity)
            elif self.tail_scales == 0:
                self._group_level(first, prev_xyz, 1 - parity)
            else:
                for S in first["scales"][self.tail_scales:]:
                    self._query_scale(first, S, prev_xyz, 1 - parity)
                    self._group_scale(first, S, prev_xyz, 1 - parity)
            if self.with_fp:
                self._interpolate_fp(1 - parity)
        for L in self.levels[(1 if self.s_first else 0):]:
            s_cur = self._sample_level(L, s_cur, parity, index_built=L is first, defer_ok=True)
        if self.with_fp:
            self._search_fp(xyz, parity)
        if self.s_query_levels:
            self._queries_of(xyz, parity)
        # if the sampling chain is the shorter stage it can take level-1 scales of stage G as its tail
        for S in first["scales"][:(0 if 0 in self.s_query_levels else self.tail_scales)]:
            self._query_scale(first, S, prev_xyz, 1 - parity)
            self._group_scale(first, S, prev_xyz, 1 - parity)
        main.wait_stream(side)

    def run_pipelined3(self, clouds, step):
        """one steady-state step of the three-stage schedule. clouds[slot] = the resident input cloud of every ring slot; this step
        samples level 1 of clouds[p] (S1), finishes the sampling chain / queries / searches of clouds[q] (S2: the batch of the step
        before) and groups clouds[r] (G: the batch of two steps before), p, q, r = step, step - 1, step - 2 mod 3. Three streams,
        forked behind the level-1 index build and joined at the end of the step: every stage reads only what the step before left."""
        p, q, r = step % 3, (step - 1) % 3, (step - 2) % 3
        main = torch.cuda.current_stream(clouds[p].device)
        side = self._side_stream(clouds[p].device)
        third = self._third_stream(clouds[p].device)
        first = self.levels[0]
        # built before the other stages are issued: a one-workgroup-per-scene kernel with 64 KB of LDS cannot find a free CU once
        # the wide kernels are in flight
        ext.scene_index_build_wrapper(self.batch, first["n"], clouds[p], first["sets"][p]["index"])
        forked = torch.cuda.Event()
        forked.record(main)
        # ---- S1 (this stream): the level-1 rounds of batch `step`
        self._deferred = self._next_built = None
        self._sample_level(first, clouds[p], p, index_built=True, defer_ok=True)
        s1_deferred = self._deferred is not None   # (a property of the configuration: the same in every step)
        s1_built = self._next_built is not None    # (likewise: level 2's index came out of the level-1 sampling call)
        self._deferred = self._next_built = None
        # ---- G: groupings (and interpolation) of the batch of two steps before
        side.wait_event(forked)
        with torch.cuda.stream(side):
            inputs = [clouds[r]] + [L["sets"][r]["new_xyz"] for L in self.levels[:-1]]
            order = list(zip(self.levels, inputs))
            for lvl, (L, cur) in enumerate(order[1:], start=1):   # feature gathers first (few registers: they share the CUs with S1)
                if lvl not in self.s_query_levels:
                    self._query_level(L, cur, r)
                self._group_scales(L, cur, r)
            if 0 not in self.s_query_levels:
                self._query_level(first, clouds[r], r)
            self._group_scales(first, clouds[r], r)
            if self.with_fp:
                self._interpolate_fp(r)
        # ---- S2: levels 2.. of the sampling chain, the ball queries and the FP searches of the batch of the step before
        third.wait_event(forked)
        with torch.cuda.stream(third):
            # what S1 of the step before left undone: the level-1 centres are gathered by level 2's index build
            self._deferred = (clouds[q], 0, q) if s1_deferred else None
            self._next_built = (1, q) if s1_built else None
            cur = first["sets"][q]["new_xyz"]
            for L in self.levels[1:]:
                cur = self._sample_level(L, cur, q, defer_ok=True)
            self._deferred = self._next_built = None
            if self.with_fp:
                self._search_fp(clouds[q], q)
            self._queries_of(clouds[q], q)
        main.wait_stream(side)
        main.wait_stream(third)

    def _third_stream(self, device):
        if getattr(self, "third", None) is None:
            self.third = torch.cuda.Stream(device=device)
        return self.third

    def _queries_of(self, xyz, parity):
        """the ball queries of the levels in s_query_levels for the batch whose centres / indices are in set `parity`"""
        cur = xyz
        for lvl, L in enumerate(self.levels):
            if lvl in self.s_query_levels:
                self._query_level(L, cur, parity)
            cur = L["sets"][parity]["new_xyz"]

    def _search_fp(self, xyz, parity):
        """three_nn + the interpolation weights of every FP level for the batch whose centres / indices are in set `parity`.
        The search is arithmetic-bound and needs nothing but coordinates, so the pipelined schedule runs it at the tail of
        stage S (the latency-bound chain leaves the chip's issue slots idle) instead of in front of the interpolation in stage G"""
        b = self.batch
        # FP modules walk back up: unknown = xyz of the finer level, known = the coarser one
        xyzs = [xyz] + [L["sets"][parity]["new_xyz"] for L in self.levels]
        # the scene index of level l's INPUT points is sets[parity]["index"] of level l
        indices = [L["sets"][parity]["index"] for L in self.levels] + [None]
        for k, F in enumerate(self.fp_bufs):
            P = F["sets"][parity if len(F["sets"]) > 1 else 0]
            known = xyzs[len(self.levels) - k]
            unknown = xyzs[len(self.levels) - k - 1]
            k_index, u_index = indices[len(self.levels) - k], indices[len(self.levels) - k - 1]
            if k_index is not None:
                ext.three_nn_indexed_wrapper(b, F["n"], F["m"], unknown, known, u_index, k_index, P["dist2"], P["idx"])
            else:
                ext.three_nn_wrapper(b, F["n"], F["m"], unknown, known, P["dist2"], P["idx"])
            inv = 1.0 / (torch.sqrt(P["dist2"]) + 1e-8)      # pointnet2_modules.py:157-159
            torch.div(inv, torch.sum(inv, dim=2, keepdim=True), out=P["weight"])
            F["dist2"], F["idx"] = P["dist2"], P["idx"]

    def _interpolate_fp(self, parity):
        b = self.batch
        for F in self.fp_bufs:
            P = F["sets"][parity if len(F["sets"]) > 1 else 0]
            ext.three_interpolate_wrapper(b, F["c"], F["m"], F["n"], F["known_feats"], P["idx"], P["weight"], F["out"])

    def _run_fp(self, xyz, parity):
        self._search_fp(xyz, parity)
        self._interpolate_fp(parity)

    def _prime(self, clouds):
        """before the first pipelined step: stage S of clouds[p] into set p for BOTH parities, so that the first step's stage G
        (the "previous batch" = clouds[1]) reads valid centres and indices, never uninitialised memory"""
        for parity in range(self.ring):
            xyz = cur = clouds[parity]
            self._deferred = self._next_built = None
            for L in self.levels:
                cur = self._sample_level(L, cur, parity, defer_ok=True)
            self._deferred = self._next_built = None
            if self.with_fp:
                self._search_fp(xyz, parity)
            if self.s_query_levels:
                self._queries_of(xyz, parity)

    def _step_eager(self, k):
        if self.stages == 3:
            self.run_pipelined3(self.inputs, k)
        elif self.pipelined:
            self.run_pipelined(self.inputs[k & 1], self.inputs[1 - (k & 1)], k)
        else:
            self.run(self.inputs[0])

    def capture(self, xyz, xyz_other=None, xyz_third=None):
        """capture the step into HIP graph(s) (torch.cuda.CUDAGraph); replay with self.replay(). Pipelined: one graph per ring slot
        (two stages: two, three stages: three), replayed in turn; graph p samples inputs[p] and works on the other slot(s) for the
        batch(es) before. `xyz` fills inputs[0], `xyz_other` / `xyz_third` (default: the same cloud) inputs[1] / inputs[2]: the
        batches the FIRST replays see as "the step(s) before"."""
        self.inputs = [xyz.clone()]
        if self.pipelined:
            self.inputs.append((xyz if xyz_other is None else xyz_other).clone())
        if self.stages == 3:
            self.inputs.append((xyz if xyz_third is None else xyz_third).clone())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        period = 1
        with torch.cuda.stream(s):
            if self.pipelined:
                self._prime(self.inputs)
        if self.pipelined:
            period = self.ring   # one graph per ring slot
        with torch.cuda.stream(s):
            for k in range(max(2, period)):   # warm-up outside capture; fills every buffer of the rotation
                self._step_eager(k)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self.graphs = []
        for k in range(period):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step_eager(k)
            self.graphs.append(g)
        self.replays = 0
        return self.graphs[0]

    def replay(self, xyz=None):
        """one step from the captured graph(s). `xyz`: the batch of THIS step, copied into the input buffer of the step's parity
        (stream-ordered behind the previous replay, the last reader of that buffer's old contents); None: the caller has
        filled stack.input_buffer() itself, or replays the resident batches again (the bench)."""
        if xyz is not None:
            self.input_buffer().copy_(xyz)
        self.graphs[self.replays % len(self.graphs)].replay()
        self.replays += 1

    def step(self, xyz):
        """eager (no graph) step on the caller's own tensor. Pipelined: stage S of `xyz` beside stage G of the cloud handed to
        the step before, which the caller therefore leaves untouched until this step has been issued (stream order does the rest)."""
        if self.stages == 3:
            if self._prev_xyz is None:
                self._prime([xyz, xyz, xyz])
                self._eager_clouds = [xyz, xyz, xyz]
                self._prev_xyz = xyz
                self.replays = 0
            self._eager_clouds[self.replays % 3] = xyz    # (the clouds of the two steps before stay referenced here)
            self.run_pipelined3(self._eager_clouds, self.replays)
            self.replays += 1
        elif self.pipelined:
            if self._prev_xyz is None:
                self._prime([xyz, xyz])
                self._prev_xyz = xyz
                self.replays = 0
            self.run_pipelined(xyz, self._prev_xyz, self.replays & 1)
            self._prev_xyz = xyz
            self.replays += 1
        else:
            self.run(xyz)

"""Batched IGLU gridworld on one MI355X: N independent envs whose state IS a set of torch
tensors in HBM, stepped by the HIP kernels behind the C ABI (include/igw.h).

Mirrors the reference's env protocol for render=False / vector_state=True
(gridworld/env.py:155-303): set_tasks -> reset -> step, with the create_env kwargs of
gridworld/env.py:333-338.  Observations are tensor views of the state, not copies.
"""
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib as L
from . import _queries as QR
from . import codec as K
from . import goal as G
from . import peek as P
from . import peek_dict as PD
from . import query as Q
from . import recall as RCL
from . import relabel as RL
from . import render as R
from . import vox as X
from . import worth as W


def _as_rows(x, device, n=None):
    """[T,9,11,11] / [T,1089] / [9,11,11] int array -> int8 tensor [T, GRID_STRIDE] on device."""
    if x is None:
        return None
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    t = t.reshape(t.shape[0], -1)
    if t.shape[1] == L.GRID_STRIDE:
        return t.to(device=device, dtype=torch.int8).contiguous()
    if t.shape[1] != L.CELLS:
        raise ValueError(f'grid rows must have 1089 cells, got {t.shape[1]}')
    out = torch.zeros((t.shape[0], L.GRID_STRIDE), dtype=torch.int8, device=device)
    out[:, :L.CELLS] = t.to(device=device, dtype=torch.int8)
    return out


def _invariant(x, n, device):
    """The `invariant` argument of a task (a bool or [n]) -> uint8 tensor [n] on device, None as it is."""
    if x is None:
        return None
    return torch.as_tensor(np.broadcast_to(np.asarray(x, dtype=np.uint8), (n,)).copy(), device=device)


class _Space:
    """The layout of one action space, stated here and nowhere else: the C entry that steps it, the entry of its fused
    action rollout (None: it has none), and per action buffer the dict key (None: the action IS the one tensor), the
    kernel's dtype and the per-env shape.  The entries take the buffers' pointers in this order."""

    def __init__(self, name, step, rollout, *buffers):
        self.name, self.step, self.rollout, self.buffers = name, step, rollout, buffers
        self.counts = tuple(int(np.prod(shape, dtype=np.int64)) for _, _, shape in buffers)   # elements per env
        self.row_bytes = tuple(dt.itemsize * n for (_, dt, _), n in zip(buffers, self.counts))

    def mismatch(self, who, N, key, x, lead=''):
        """The one error for a buffer that does not fit the layout (`lead`: 'T' for [T, N, ...] sequences)."""
        layout = ', '.join(f'{k or "actions"} {dt} [{", ".join(map(str, (*lead, N, *shape)))}]'
                           for k, dt, shape in self.buffers)
        return ValueError(f'{who}: the {self.name} action space takes {layout}, got {key or "actions"} {tuple(x.shape)}')


_SPACES = {
    L.WALKING_DISCRETE: _Space('walking', 'igw_step_walking', 'igw_rollout_walking_actions', (None, torch.int32, ())),
    L.WALKING_DICT: _Space('walking Dict', 'igw_step_walking_dict', None,
                           ('buttons', torch.uint8, (8,)), ('camera', torch.float32, (2,))),
    L.FLYING: _Space('flying', 'igw_step_flying', 'igw_rollout_flying_actions',
                     ('movement', torch.float32, (3,)), ('camera', torch.float32, (2,)),
                     ('inventory', torch.int32, ()), ('placement', torch.int32, ())),
}
BUTTONS = ('forward', 'back', 'left', 'right', 'jump', 'attack', 'use', 'hotbar')   # the reference's keys, env.py:60-70
# the fields of L.Buffers in their order (the per-env ones are bound by row range), without `stats`
_ROW_BUFFERS = ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf')
_TASK_BUFFERS = ('task_target', 'task_start', 'task_start_occ', 'task_meta', 'task_index')


class _FillFlag:
    """"The next draw restarts the stack" (pov_obs): ONE holder per batch, on the VecGridWorld; its sub-batches and the
    device reach it through here.  The fact is kept per row range that draws (the whole batch, each sub-batch): `drawn`
    holds the ranges that have drawn since the state last moved without a draw, so the first draw of EACH range after
    such a move fills.  raise_() -- whatever moved the state without drawing; take() -- an eager draw of a range;
    captured() -- the first draw of a captured chain, which cannot read the host at replay time: from the first capture
    on the flag is also one byte per env on the device (row 0 of `dev`; row 1 is the restart mask the captured draw
    reads).  The bytes are lowered by the whole batch's draws and by replays, not by a sub-batch's eager draw (which
    launches nothing but its draw on its stream)."""

    def __init__(self, n, device):
        self.drawn, self.dev, self.n, self.device = weakref.WeakSet(), None, n, device

    def raise_(self):
        self.drawn.clear()
        if self.dev is not None:
            self.dev[0].fill_(1)

    def take(self, rows):
        """Whether the eager draw of the range `rows` that is about to be launched fills; lowers its flag."""
        fill = rows not in self.drawn
        if fill:
            self.lowered(rows)
            if rows.parent is None and self.dev is not None:
                self.dev[0].zero_()
        return fill

    def lowered(self, *ranges):
        """These ranges need no fill: a replayed graph's first draws took their flags; a new sub-batch of a batch
        that has drawn."""
        self.drawn.update(ranges)

    def on_device(self, root):
        """(Before a capture: nothing may be allocated inside one.)"""
        if self.dev is None:
            self.dev = torch.zeros((2, self.n), dtype=torch.uint8, device=self.device)
            self.dev[0].fill_(int(root not in self.drawn))

    def captured(self, sl, restart):
        """The captured form of take(): the restart mask of a replay's first draw of rows `sl` -- the eager rule's
        `restart` (a uint8 tensor or None) OR the flag bytes as they are at replay time -- computed and the bytes
        lowered by launches that are captured with the draw."""
        first, mask = self.dev[0, sl], self.dev[1, sl]
        if restart is None:
            mask.copy_(first)
        else:
            torch.bitwise_or(restart, first, out=mask)
        first.zero_()
        return mask


class _Rows:
    """Rows [lo, lo + n) of a batch's state behind one igw context, and what follows that state: the base of
    VecGridWorld (every row, launches on the current stream) and SubBatch (a slice of its parent's tensors, launches on
    a stream of its own).  The two differ by `parent`, `lo` and `stream` alone."""
    parent, lo, stream = None, 0, None

    def _root(self):
        return self if self.parent is None else self.parent

    def _open(self, cfg, stats_buf):
        """Creates the context of `cfg` over this row range of the root's buffers."""
        root, sl = self._root(), slice(self.lo, self.lo + cfg.num_envs)
        self.cfg, self.num_envs, self.env_index_base, self.stats_buf = cfg, cfg.num_envs, cfg.env_index_base, stats_buf
        self.ctx = C.c_void_p()
        L.check(self.lib.igw_create(C.byref(cfg), C.byref(self.ctx)), 'igw_create')
        bound = [getattr(root, k)[sl] for k in _ROW_BUFFERS] + [getattr(root, k) for k in _TASK_BUFFERS] + \
            [root.out_buf[sl], stats_buf]
        L.check(self.lib.igw_bind_buffers(self.ctx, C.byref(L.Buffers(*[t.data_ptr() for t in bound]))),
                'igw_bind_buffers')
        self._sl = sl
        self._rows = (root.agent_buf[sl], root.grid_buf[sl], root.occ_buf[sl])   # the state a frame is drawn from

    def _follow_with(self, pov, mask, goal=None, vox=None):
        """The persistent tensors that follow the state (a _Pov or None; obs['action_mask'] or None; the dict of the
        goal query's outputs or None; the (VoxSpec, obs['vox_obs']) pair or None): this range's rows of them, and the
        observation dict that holds them beside the state's views."""
        self._pov, self._mask, self._goal, self._vox = pov, mask, goal, vox
        self.pov = pov.tensors.get('rgb') if pov else None
        self.pov_obs = pov.obs if pov else None
        self._obs = {'agentPos': self.agent_pos, 'inventory': self.inventory, 'compass': self.compass.unsqueeze(1),
                     'grid': self.grid}
        if pov is not None:
            pov.add_to(self._obs)
        if mask is not None:
            self._obs['action_mask'] = mask
        if goal is not None:
            self._obs.update(goal)
            if 'gain' in goal:
                self._goal_scratch()   # (before the first launch that follows, which may be a captured one)
        if vox is not None:
            self._obs['vox_obs'] = vox[1]

    def __del__(self):
        ctx = getattr(self, 'ctx', None)
        if ctx:
            self.lib.igw_destroy(ctx)
            self.ctx = None

    def _stream(self):
        if self.stream is None:
            return C.c_void_p(torch._C._cuda_getCurrentRawStream(self._dev_index))
        return C.c_void_p(self.stream.cuda_stream)

    def _in_use(self, *tensors):
        """Marks tensors as in use on the range's own stream, so that the caching allocator does not recycle them while
        a launch there reads or writes them; on the current stream there is nothing to mark."""
        if self.stream is not None:
            for t in tensors:
                if torch.is_tensor(t):
                    t.record_stream(self.stream)

    def _query(self, rows, *args, out=None, also=()):
        """One query call that returns a dict of tensors: marks `out`'s tensors (and `also`) as in use on the range's
        stream, calls the adapter `rows` of _queries there, marks what it returns and returns it."""
        self._in_use(*also, *(out or {}).values())
        res = rows(self, *args, out, self._stream(), self.stream)
        self._in_use(*res.values())
        return res

    def _atlas(self):
        root = self._root()
        if root._render_atlas is None:
            root.set_render_atlas(None)
        return root._render_atlas

    def obs(self):
        return self._obs.copy()

    # ---- what follows a launch ----
    def _follow(self, restart=None, fill=False, draw=True):
        """The ONE path after a launch that moved this range's state: the draw (renderer='hip'), then the action mask
        (action_mask=True), then the goal query (goal=...), then the voxel observation (vox_obs=..., which may read the
        goal's rows), on the range's stream.
        `restart` / `fill` are the stacks' restart rule of the draw and of the voxel observation
        (pov_obs, vox_obs; ignored without): a uint8 tensor [n] of the rows to restart -- a step's _ended(),
        reset(mask)'s mask -- or fill=True for every row (a full reset); the range's first draw after an undrawn move
        fills too (ONE flag for both stacks, taken once: they are written by the same calls).
        draw=False is the move that draws nothing (the fused rollouts, load_state_dict): it raises that flag."""
        stacks = (self._pov is not None and self._pov.obs is not None) or self._vox is not None
        if not draw:
            self._root()._fill.raise_()
        elif stacks:
            fill = self._root()._fill.take(self) or fill
        if draw and self._pov is not None:
            self._draw(None, restart, fill)
        self._follow_mask()
        self._follow_goal()
        if draw and self._vox is not None:
            self._write_vox(None, restart, fill)

    def _follow_captured(self, stream, first, last):
        """_follow() after a step inside a captured chain, on the capture's stream (`first` / `last`: of the chain's
        steps).  A stack of K > 1 frames takes every step's frame, so the draw follows each step, the first with the
        captured form of the restart rule (_FillFlag.captured); otherwise one draw follows the last step's mask --
        what the eager loop's last step() leaves."""
        pov, vox = self._pov, self._vox
        pov_stacked, vox_stacked = pov is not None and pov.stacked, vox is not None and vox[0].stack > 1
        if pov_stacked or vox_stacked:   # (one captured mask for both stacks, as _follow takes the flag once)
            restart = self._ended()
            if first:
                restart = self._root()._fill.captured(self._sl, restart)
        if pov_stacked:
            self._draw(stream, restart)
        self._follow_mask(stream)
        self._follow_goal(stream)
        if last and pov is not None and not pov.stacked:
            self._draw(stream)
        if vox_stacked:
            self._write_vox(stream, restart)
        elif last and vox is not None:
            self._write_vox(stream)

    def _follow_mask(self, stream=None):
        if self._mask is not None:
            QR.mask_rows(self, self._mask, False, None, self._stream() if stream is None else stream)

    def _follow_goal(self, stream=None):
        if self._goal is not None:
            QR.goal_rows(self, tuple(self._goal), self._goal, self._stream() if stream is None else stream,
                         captured=stream is not None)

    def _goal_scratch(self):
        """What gain=True needs beside its outputs, allocated once per range (on its stream) and kept, so that later
        calls allocate nothing: the mask and look tensors of igw_action_mask, a copy of the agent records and a mask
        nobody reads (_queries.goal_rows)."""
        tmp = getattr(self, '_goal_tmp', None)
        if tmp is None:
            n, dev = self.num_envs, self.device
            with torch.cuda.stream(self.stream):
                tmp = self._goal_tmp = (torch.zeros((n, Q.ACTIONS), dtype=torch.uint8, device=dev),
                                        torch.zeros((n, 2), dtype=torch.int16, device=dev),
                                        torch.zeros((n, L.AGENT_BYTES), dtype=torch.uint8, device=dev),
                                        torch.zeros((n, Q.ACTIONS), dtype=torch.uint8, device=dev))
        return tmp

    def _ended(self):
        """The stacks a step's draw restarts: those of the envs whose episode just ended if they auto-reset (the frame
        then shows the next episode), none otherwise (the terminal frame joins its own episode's stack)."""
        return self.done if self.autoreset else None

    def _draw(self, stream=None, restart=None, fill=False):
        """Draws the persistent outputs from this range's state rows on `stream` (a capture's); without one on the
        range's own, where the tensors are then marked as in use.  `restart` (None or a uint8 tensor [n] at any
        stride) and `fill` go to igw_render_pov_obs; ignored without pov_obs."""
        pov = self._pov
        if stream is None:
            stream = self._stream()
            self._in_use(*pov.tensors.values(), pov.obs)
        if pov.obs is not None:
            _render_obs_rows(self, pov.spec, pov.obs, pov.tensors.get('rgb'), restart, fill, stream)
        elif pov.plain:
            _render_rows(self, pov.tensors['rgb'], 3, None, None, stream)
        else:
            _render_rows(self, pov.tensors, 3, None, tuple(pov.tensors), stream)

    def _write_vox(self, stream=None, restart=None, fill=False):
        """Writes obs['vox_obs'] from this range's state rows (and its rows of the goal's planes) on `stream` (a
        capture's); without one on the range's own, where the tensor is then marked as in use."""
        spec, data = self._vox
        if stream is None:
            stream = self._stream()
            self._in_use(data)
        QR.vox_rows(self, spec, data, restart, fill, self._goal, stream)

    def step_walking_ptr(self, actions_i32):
        """Hot-loop variant: `actions_i32` is already a contiguous int32 device tensor [n], launched on the range's
        stream (on a stream of its own the tensor is marked as in use there).  With action_mask=True the mask follows.
        The WHOLE batch's call does NOT draw: obs['pov'] and the other render outputs keep what the last step() /
        reset() left; a SubBatch's draws, as step() does."""
        if actions_i32.numel() != self.num_envs:
            raise _SPACES[L.WALKING_DISCRETE].mismatch('step_walking_ptr', self.num_envs, None, actions_i32)
        self._in_use(actions_i32)
        L.check(self.lib.igw_step_walking(self.ctx, actions_i32.data_ptr(), self._stream()), 'igw_step_walking')
        # The one asymmetry between the two classes, decided here: a sub-batch has no step() of its own, so this is
        # its step and it draws; the whole batch's never drew (and, not being an undrawn MOVE of the episode
        # boundaries, it leaves the stacks' fill flag alone): its callers draw when they want a frame.
        if self.parent is None:
            self._follow_mask()
            self._follow_goal()
        else:
            self._follow(self._ended())

    # ---- which actions would act (libigw_query.so, include/igw_query.h) ----
    def action_mask(self, out=None, look=False, sample=None):
        """Which of the 18 walking actions would act on every env's CURRENT state (after a step that ended an episode of
        an auto-reset env: the new episode's): uint8 [N, 18], 1 where the action would do something -- the place / break
        / hotbar actions would change the grid, a jump would start, the pitch would move; the no-op, the moves and the
        yaw actions are always 1 (names in query.ACTION_NAMES).  One igw_action_mask launch on the
        range's stream (a VecGridWorld's: the current one; a SubBatch's: its own, for its rows); with `out` (a
        contiguous uint8 device tensor of that shape) nothing is allocated, so the call
        can be captured.  look=True also returns int16 [N, 2]: the grid cell (index into the flat [9 * 11 * 11] grid)
        that action 16 would clear and the one action 17 would fill, -1 where they would do nothing.  sample=(seed, t)
        also returns int32 [N]: one action per env drawn uniformly from the set bits of its mask, a counter RNG keyed by
        (seed, global env index, t) (include/igw_query.h) -- a masked random policy without a host round trip.  The
        result is the mask alone or the tuple (mask, look, actions) of what was asked for; with look / sample `out` may
        be the tuple of tensors to write.  Discrete(18) walking only: ValueError for flying and Dict-action envs."""
        self._in_use(*(out if isinstance(out, (tuple, list)) else (out,)))
        res = QR.mask_rows(self, out, look, sample, self._stream(), self.stream)
        self._in_use(*(res if isinstance(res, tuple) else (res,)))
        return res

    # ---- where the reward wants the target (libigw_goal.so, include/igw_goal.h) ----
    def goal(self, want=False, todo=True, gain=False, out=None):
        """Where the reward currently wants the target, what is left of it and -- gain=True -- what every action would
        earn, for every env's CURRENT state: a dict of
          align int8 [N, 3]    (dx, dz, rot) = Task.argmax_intersection of the live synthetic grid
          fit   int16 [N, 4]   (max_int, target_size, size, cached_max_int)
          want  int8 [N, 9, 11, 11] (want=True)   the synthetic target under that alignment, in the grid's frame
          todo  int8 [N, 9, 11, 11] (todo=True)   want where the synthetic grid differs from it, else 0
          gain  float32 [N, 18], ends uint8 [N, 18] (gain=True)   the reward and `done` that step(a) would return
        want / todo are strided views of 1104-byte rows, as `grid` is.  One igw_goal launch on the range's stream;
        gain=True first launches igw_action_mask there (twice: the mask of the state, and the cells of a copy of the
        agent records with a full inventory, so that a colour that can be placed where the active one cannot has its
        cell), into scratch tensors the range keeps.  `out`: a dict of tensors to write, as an earlier call returned
        them; with every output given nothing is allocated (gain=True: from the range's second such call on), so the
        call can be captured.  align / fit / want / todo work in every action space; gain=True raises ValueError
        outside Discrete(18) walking and with size_reward=True (the wrapper's reward is not what is predicted)."""
        names = ('align', 'fit') + (('want',) if want else ()) + (('todo',) if todo else ()) + \
            (('gain', 'ends') if gain else ())
        return self._query(QR.goal_rows, names, out=out)

    # ---- which cells a turn of the camera reaches (libigw_aim.so, include/igw_aim.h) ----
    def aim(self, max_turns=72, place=True, brk=True, out=None):
        """Which grid cells a place / a break can reach from every env's CURRENT position by turning the camera alone, and
        the cheapest turn that gets there: a dict of 'place' and 'break' (place=True / brk=True),
        each int32 [N, 9, 11, 11] -- per cell the code turns << 16 | (dpitch_steps + 36) << 8 | (dyaw_steps + 36) of the
        cheapest camera direction within `max_turns` (0..72) 5-degree camera actions whose sight ray would fill / clear
        that cell, -1 where there is none (aim_decode, aim_action).  Inventory and the active block are not looked at.
        The planes are strided views of 1104-word rows, as `grid` is of its rows.  One igw_aim launch on the range's
        stream; `out`: a dict of planes to write, as an earlier call returned them; with every plane given nothing is
        allocated, so the call can be captured.  Discrete(18) walking only: ValueError for flying and Dict-action envs,
        for a max_turns outside 0..72 and with both planes off."""
        return self._query(QR.aim_rows, max_turns, place, brk, out=out)

    # ---- K action sequences of H steps from the live state (libigw_peek.so, include/igw_peek.h) ----
    def peek(self, actions, gamma=1.0, outputs=P.OUTPUTS, out=None):
        """What every env would be paid, when its episode would end, what it would build and where it would stand if it
        played each of K sequences of H actions from its CURRENT state, which is not touched.
        `actions`: an integer tensor or array [K, H] (the same sequences for every env) or [N, K, H], 1 <= K <= 4096,
        1 <= H <= 32; converted to a contiguous int32 device tensor only if it is not one already (a value outside 0..17 of
        any integer width is a no-op).  A dict of the
        `outputs` named:
          reward float32 [N, K, H]   the reward of step h, +0.0 after the candidate ended
          ends   int16 [N, K]        h + 1 of the step that returned done, 0 if none did
          change int16 [N, K, H]     colour << 11 | cell of the cell step h changed, -1 for none (peek_decode)
          pose   float32 [N, K, 5]   agentPos after the last executed step
          ret    float32 [N, K]      the return discounted by `gamma`, summed in binary64 (peek_best)
        Every step is bit for bit the step's own; a candidate ends with the first step that returns done and no reset
        is simulated.  One igw_peek launch on the range's stream; `out`: a dict of tensors to write, as an earlier call
        returned them; with every output given nothing is allocated, so the call can be captured.  ValueError outside
        Discrete(18) walking, with size_reward=True (the wrapper's reward is not what is predicted), for K or H out of
        range, a wrong rank, a first dimension that is not N, and for empty or unknown outputs."""
        names = P.check_outputs(outputs)
        return self._query(QR.peek_rows, actions, gamma, names, out=out)

    # ---- ... of the flying and the walking Dict spaces (libigw_peek_dict.so, include/igw_peek_dict.h) ----
    def peek_dict(self, actions, gamma=1.0, outputs=PD.OUTPUTS, out=None):
        """peek() for the flying and the walking Dict (discretize=False) action spaces: what every
        env would be paid, when its episode would end, what it would build and where it would stand if it played each of
        K sequences of H actions from its CURRENT state, which is not touched.  `actions`: a dict with the keys of the
        env's own step() -- flying: movement [.., 3], camera [.., 2], inventory [..], placement [..]; walking Dict:
        buttons [.., 8] (forward, back, left, right, jump, attack, use, hotbar), camera [.., 2] -- every entry behind
        the same leading shape [K, H] (the same sequences for every env) or [N, K, H], 1 <= K <= 4096, 1 <= H <= 32;
        an entry is converted to a contiguous device tensor of the step's dtype (float32, int32, uint8) only if it is
        not one already.  An invalid component of an action (a value that is not finite, a camera delta beyond
        +-1e6, an inventory / hotbar id outside 0..6, a placement outside 0..2) runs as the no-op the step makes of it;
        nothing is counted.  Returns peek()'s dict of the `outputs` named (reward, ends, change, pose, ret; peek_decode
        and peek_best read it).  One launch on the range's stream; `out`: a dict of tensors to write, as an earlier call
        returned them; with every output given and the actions already such device tensors nothing is allocated, so
        the call can be captured.  ValueError in the Discrete(18) space (that is env.peek), with size_reward=True,
        for missing or extra keys, leading shapes that differ, K or H out of range, a wrong rank, a first dimension
        that is not N, and for empty or unknown outputs."""
        names = PD.check_outputs(outputs)
        return self._query(QR.peek_dict_rows, actions, gamma, names, out=out)

    # ---- what every single-cell edit would be paid (libigw_worth.so, include/igw_worth.h) ----
    def worth(self, outputs=W.OUTPUTS, allow=None, stocked=False, out=None):
        """What the env would pay for every single-cell edit of every env's CURRENT state, which is not touched (DESIGN.md
        section 16): a dict of the `outputs` named,
          word int16 [N, 7, 9, 11, 11]   plane 0: break the cell, planes 1..6: place that colour in it (worth_plane_names);
                                         right | (wrong + 1) << 12 | ends << 14, -1 where the edit is invalid (a break of
                                         an empty cell, a place into a full one); worth_decode reads it
          best int32 [N, 4]              (plane, cell, word, candidates) of the best-paid edit, (-1, -1, -1, 0) without one
        `word` is a strided view of seven 1104-word rows per env, each in the layout of `grid`.  `best` is chosen among
        the valid edits that pass two gates, neither of which changes `word`: `allow`, a uint8 device tensor [N, 2, 9,
        11, 11] with 1104-byte rows (worth.allow_from_aim builds it from aim()'s planes) or contiguous [N, 2, 1104] --
        plane 0 gates the breaks of a cell, plane 1 the places into it -- and stocked=True, which leaves out the colours
        whose inventory is empty.  Inventory, adjacency, the agent's overlap and reach do not gate validity.  One
        igw_worth launch on the range's stream; `out`: a dict of tensors to write, as an earlier call returned them;
        with every output given nothing is allocated, so the call can be captured.  Every action space; SizeReward's
        reward is not predicted.  ValueError for empty or unknown outputs, a wrong `out` and a wrong `allow`."""
        names = W.check_outputs(outputs)
        return self._query(QR.worth_rows, names, allow, stocked, out=out, also=(allow,))

    # ---- rewards of logged episodes under other targets (libigw_relabel.so, include/igw_relabel.h) ----
    def relabel(self, goals='final', gamma=1.0, outputs=RL.DEFAULT, out=None):
        """Hindsight relabelling of the episode log (enable_trajectory_log / EpisodeLogger): for
        every logged env of this range, E of them, the reward, done and return its most recent FINISHED episode would
        have had under each of G other targets.  `goals`: 'final' (the grid the episode ended with), 'own' (the episode's
        own target, task_target + task_start of its task row: it reproduces the logged rewards), an integer tensor
        [E, G] of entries of the episode itself (0 = its start, its length = its final grid; relabel_future draws HER's
        "future" entries), or a tensor of targets [E, G, 9, 11, 11] / [E, G, 1104].  A dict of the `outputs` named --
          reward float32 / done uint8 / progress int16 [E, G, L]   per step, +0 past the episode's length (L = the log's
                                                                    capacity; progress is the cached max_int)
          end int32 [E, G], ret float32 [E, G]                      the first done step (0: none) and the return
                                                                    discounted by `gamma` up to it
          target_size int16 [E, G], target int8 [E, G, 9, 11, 11]   the goals used (vox_obs / render_views read them)
        -- plus length int32 [E] and valid uint8 [E]: 0 for an env without a finished episode, whose rows are padding.
        Slots, lengths and starting rows come from the log's heads and the task table with torch operations on the
        range's stream and the kernel reads only the records' change words: no env state is touched and the host never
        waits, so the call can be captured.  It uses the env's scales and max_steps, every action space; like the log's
        grids it reads the episode's task row, so a set_tasks (or the RandomTasks generator) that rewrote the row since
        changes the start.  ValueError without a log, for a range that holds no logged env, with size_reward=True, and
        for empty or unknown outputs or a wrong `out`."""
        names = RL.check_outputs(outputs)
        return self._query(QR.relabel_rows, goals, gamma, names, out=out)

    # ---- voxel observations of logged transitions (libigw_recall.so, include/igw_recall.h) ----
    def recall(self, spec, batch=None, seed=0, episode=None, step=None, goals=None, goal=None, outputs=RCL.ENV_DEFAULT,
               out=None):
        """A minibatch of logged transitions in the layout `spec` (a vox.VoxSpec or a dict of its arguments with the
        planes 'grid' and 'target'): for B samples (e, t) -- step t of the most recent FINISHED
        episode of the e-th logged env of this range -- obs and next_obs [B, K * C, 9, S, S], what a vox_obs stack of K
        showed before and after the step, rebuilt from the log's change words and float32 poses by one igw_recall launch
        on the range's stream.  Samples: `episode` and `step` ([B] integers, 1 <= step <= length), or `batch` of them
        drawn with a torch generator seeded by `seed` (the env uniform, the step uniform over its episode).  A 'target'
        plane shows the sample's goal: goals='own' (task_target + task_start of the episode's task row) or goals=r, the
        dict relabel() returned with 'target', and `goal` [B], the column g of each sample (default 0); with r's 'reward'
        / 'done' the result also holds reward_relabel / done_relabel [B], r's values at (e, g, t - 1).  A dict of the
        `outputs` named -- obs, next_obs, record uint8 [B, 64] with recall.decode()'s views of it (action, reward, done,
        inventory, agent_pos), valid uint8 [B] -- plus episode and step int32 [B].  A sample out of range, or of an env
        without a finished episode, is padding: valid 0, its observations all `bias`, its record zeros.  Starts and reset
        poses come from the task table by the head's task row with torch operations on the range's stream: no env state is
        touched and the host never waits, so the call can be captured (with `episode` / `step` given: a torch generator
        does not draw inside a capture); `out`: a dict of tensors to write, as an earlier call returned them.  Every
        action space.  The poses are the LOG's (float32): next to a half-integer coordinate the
        head cell can differ from the one the live vox_obs showed.  ValueError without a log, for a range that holds no
        logged env, for 'want' / 'todo' planes, a 'target' plane without goals, and a wrong `out`."""
        spec, _ = RCL.spec_of(spec)
        names = RCL.check_outputs(outputs)
        return self._query(QR.recall_rows, spec, batch, seed, episode, step, goals, goal, names, out=out)

    # ---- the state as the tensor a policy network reads (libigw_vox.so, include/igw_vox.h) ----
    def vox_obs(self, spec, out=None, restart=None, fill=False, goal=None):
        """Every env's CURRENT state in the layout `spec` (a vox.VoxSpec or a dict of its arguments; DESIGN.md section
        14): a [N, K * C, 9, S, S] tensor of spec.dtype -- channel-first one-hot / occupancy planes of the grid, the
        target and the goal query's rows, the agent's body, in the world's or the agent's frame, the last K calls
        stacked.  One igw_vox_obs launch on the range's stream that shifts the new planes into `out` (the tensor an
        earlier call returned), restarting the stack of env i where `restart` (a uint8 / bool device tensor [N], any
        stride) is not 0, of every env with fill=True.  out=None returns a new, filled tensor; with `out` nothing is
        allocated, so the call can be captured.  'want' / 'todo' planes are read from `goal`, the dict
        goal(want=True, todo=True) returned (ValueError without it).  Every action space."""
        spec = X.VoxSpec.of(spec)
        if restart is not None and not (torch.is_tensor(restart) and restart.dtype in (torch.uint8, torch.bool)):
            with torch.cuda.stream(self.stream):
                restart = torch.as_tensor(restart, device=self.device).ne(0).to(torch.uint8)
        self._in_use(out, restart, *(goal or {}).values())
        res = QR.vox_rows(self, spec, out, restart, fill, goal, self._stream(), self.stream)
        self._in_use(res)
        return res

    # ---- first-person frames (libigw_render.so, include/igw_render.h) ----
    def render_pov(self, out=None, channels=3, size=None, outputs=None, codec=None, quality=90):
        """The first-person frame of every env's CURRENT state (see _make_views for auto-reset envs): uint8
        [N, H, W, channels] with W, H = size (default render_size), row 0 the top image row, channels 3 (RGB) or 4 (RGBA,
        what the reference's Renderer.render() returns).  One launch on the range's stream (a VecGridWorld's: the
        current one; a SubBatch's: its own, for its rows); with `out` (a contiguous
        uint8 device tensor of that shape) nothing is allocated, so the call can be captured in a graph.
        outputs (a tuple of 'rgb', 'depth', 'label', 'surface') returns a dict name -> tensor instead, from one
        igw_render_pov_aux launch: the frame and / or the [N, H, W] planes float32 depth, uint8 label, int16 surface
        (include/igw_render.h); `out` is then a dict of preallocated tensors under those names, or None.
        codec='jpeg' returns (buf, sizes) of codec.encode_jpeg instead: the frames are drawn, then encoded at `quality`
        by a second launch on the same stream; `out` is then the (buf, sizes) pair to encode into, or None."""
        self._in_use(*(out.values() if isinstance(out, dict) else out if isinstance(out, (tuple, list)) else (out,)))

        def draw(out=None, outputs=None):
            return _render_rows(self, out, channels, size, outputs, self._stream(), self.stream)
        with torch.cuda.stream(self.stream):
            res = K.encoded(codec, outputs, quality, out, draw)
        if res is None:
            return draw(out, outputs)
        self._in_use(*res)
        return res


class VecGridWorld(_Rows):
    """N envs on one GPU.  kwargs follow create_env (gridworld/env.py:333-338)."""

    def __init__(self, num_envs, device='cuda:0', action_space='walking', select_and_place=True,
                 size_reward=True, max_steps=250, right_placement_scale=1., wrong_placement_scale=0.1,
                 discretize=True, autoreset=False, num_tasks=None, lanes_per_env=0, debug_flags=0, env_index_base=0,
                 host_records=False, render=False, render_size=(64, 64), target_in_obs=False, vector_state=True, name='', fake=False,
                 renderer=None, pov_outputs=('rgb',), pov_obs=None, pov_frame=True, action_mask=False, goal=False,
                 vox_obs=None):
        """create_env's keyword arguments (gridworld/env.py:333-338) plus the batch's own: num_envs, device,
        autoreset (reset inside step), num_tasks (rows of the task table, default num_envs), lanes_per_env
        (0 = automatic), env_index_base (global index of env 0: rank / sub-batch offset), debug_flags (IGW_DIAG
        build only), host_records (the output / agent / aux records and the grid live in PINNED HOST memory that the
        kernels read and write across PCIe: a host-side consumer of a FEW envs -- the 1-env gym facade -- then needs no
        copy at all, only a stream synchronisation; the observation tensors are CPU tensors in that case).  Anything else is a TypeError, as in create_env.  render / render_size / fake / name /
        target_in_obs / vector_state are accepted for signature compatibility: this is the render=False,
        vector_state=True path (observations are the state tensors; `targets()` gives the target grids).
        renderer='hip' adds the reference's first-person frame: reset() / step() also return obs['pov'], a uint8
        [N, H, W, 3] device tensor (W, H = render_size) rendered by libigw_render.so on the same stream after the
        step / reset launch, the same tensor every call (render_pov(), DESIGN.md "First-person frames").
        pov_outputs (with renderer='hip') names what that launch writes: 'rgb' is obs['pov']; 'depth' (float32),
        'label' (uint8) and 'surface' (int16) add obs keys of those names, persistent [N, H, W] planes rewritten by
        every reset() / step() in the same launch (include/igw_render.h: igw_render_aux).  The default, ('rgb',), is
        obs['pov'] alone.
        pov_obs (with renderer='hip'; a render.ObsSpec or a dict of its arguments) adds obs['pov_obs'], the observation
        a policy network reads: a persistent [N, K * planes, H, W] tensor of the spec's dtype -- channel-first, grey or
        RGB, scaled, the last K frames stacked -- written by the one launch that draws obs['pov']
        (include/igw_render_obs.h: igw_render_pov_obs).  The env owns the stack's episode boundaries: reset() fills every env's stack with its
        frame, reset(mask) the masked envs', step() with autoreset=True those of the envs whose episode just ended (the
        frame drawn then already shows the next episode), step() with autoreset=False none (the terminal frame joins
        its own episode's stack); after anything that moves the state without drawing (rollout, rollout_actions,
        load_state_dict, set_tasks) the next draw fills.  pov_frame=False (only with pov_obs) drops obs['pov'] and its
        store.  pov_obs goes with pov_outputs=('rgb',) only.
        action_mask=True (Discrete(18) walking only) adds obs['action_mask'], a persistent uint8 [N, 18] tensor: which
        actions would act on the state the observation shows (action_mask()), written by one
        igw_action_mask launch on the same stream after the step / reset launch (and after the draw).
        goal=True, or a tuple of 'want', 'todo', 'gain' (True = ('todo',)), adds obs['align'], obs['fit'] and the
        outputs named (gain: obs['gain'] and obs['ends']): persistent tensors of goal()'s layout, rewritten by one
        igw_goal launch after the mask's.  'gain' has goal(gain=True)'s conditions.
        vox_obs (a vox.VoxSpec or a dict of its arguments) adds obs['vox_obs'], the state as the tensor a policy
        network reads (vox_obs()): a persistent [N, K * C, 9, S, S] tensor of the spec's dtype,
        rewritten by one igw_vox_obs launch after the goal's.  Its 'want' / 'todo' planes are the goal query's, so
        `goal` has to name them.  The stack's episode boundaries are pov_obs's: reset() fills, reset(mask) the masked
        envs, step() with autoreset=True the envs whose episode just ended, with autoreset=False none; after anything
        that moves the state without following (rollout, rollout_actions, load_state_dict, set_tasks) the next write
        fills."""
        if renderer not in (None, 'hip'):
            raise ValueError(f"unknown renderer {renderer!r}; the one renderer is 'hip'")
        pov_outputs = R.check_outputs(pov_outputs)
        if renderer is None and pov_outputs != ('rgb',):
            raise ValueError("pov_outputs needs renderer='hip'")
        if pov_obs is not None:
            if renderer is None:
                raise ValueError("pov_obs needs renderer='hip'")
            if pov_outputs != ('rgb',):
                raise ValueError("pov_obs goes with pov_outputs=('rgb',) only: the planes are not written in this layout")
            pov_obs = R.ObsSpec.of(pov_obs)
        elif not pov_frame:
            raise ValueError('pov_frame=False needs pov_obs (there would be nothing to draw)')
        if vox_obs is not None:
            vox_obs = X.VoxSpec.of(vox_obs)
            held_names = ('todo',) if goal is True else tuple(goal or ())
            lack = [k for k in vox_obs.needs() if k not in held_names]
            if lack:
                raise ValueError(f"vox_obs reads the goal query's {lack}: name them in goal= (goal={tuple(lack)!r})")
        if render and not fake and renderer is None:
            raise NotImplementedError("render=True needs renderer='hip' (the batched HIP ray caster of the "
                                      "first-person frame); or pass render=False")
        if not torch.cuda.is_available():
            raise L.IgwError('VecGridWorld needs a HIP device (no CPU fallback)')
        if action_space not in ('walking', 'flying'):
            raise ValueError(f'unknown action_space {action_space!r}')
        if action_mask and (action_space != 'walking' or not discretize):
            raise ValueError('action_mask=True needs the Discrete(18) walking action space')
        self.lib = L.load()
        self.device = torch.device(device)
        self.num_envs = int(num_envs)
        self.num_tasks = int(num_tasks or num_envs)
        self.flying = action_space == 'flying'
        self.walk_dict = action_space == 'walking' and not discretize
        mode = L.FLYING if self.flying else L.WALKING_DICT if self.walk_dict else L.WALKING_DISCRETE
        self._space = _SPACES[mode]
        self.max_steps = int(max_steps)
        self.autoreset = bool(autoreset)
        self.select_and_place = bool(select_and_place)
        N, T, dev = self.num_envs, self.num_tasks, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        # What a host-side consumer reads back after a step -- output, agent and aux records, the grid -- comes from ONE
        # allocation (`host_view`), so the 1-env facade moves it with a single device-to-host copy (gridworld_amd/env.py)
        rec = L.OUT_BYTES + L.AGENT_BYTES + L.AUX_BYTES
        self.host_records = bool(host_records)
        if self.host_records:   # pinned, device-mapped host memory (hipHostMalloc): the same address on both sides
            self.host_view = torch.zeros((N * (rec + L.GRID_STRIDE),), dtype=torch.uint8).pin_memory()
        else:
            self.host_view = z((N * (rec + L.GRID_STRIDE),), torch.uint8)
        cut = lambda lo, width: self.host_view[N * lo:N * (lo + width)].view(N, width)  # noqa: E731
        self.out_buf = cut(0, L.OUT_BYTES)         # agentPos, inventory, compass, reward, done of every step
        self.agent_buf = cut(L.OUT_BYTES, L.AGENT_BYTES)   # pose, inventory, step_no, pack (include/igw.h)
        self.aux_buf = cut(L.OUT_BYTES + L.AGENT_BYTES, L.AUX_BYTES)   # size, prev_size, max_int, target_size, task, episode
        self.grid_buf = cut(rec, L.GRID_STRIDE).view(torch.int8)
        self.occ_buf = z((N, L.OCC_WORDS), torch.int32)
        self.hist_buf = z((N, L.HIST_ROW), torch.int16)
        self.task_target = z((T, L.GRID_STRIDE), torch.int8)
        self.task_start = z((T, L.GRID_STRIDE), torch.int8)
        self.task_start_occ = z((T, L.OCC_WORDS), torch.int32)
        self.task_meta = z((T, L.TASK_META_BYTES), torch.uint8)
        self.task_index = z((T, L.TASK_INDEX_BYTES), torch.uint8)   # colour index of the synthetic targets (include/igw.h)
        self._make_views()
        # Agent.__init__ (core/world.py:12-29): time_int_steps = 2, active_block = BLUE, inventory 20
        self.agent_buf.view(torch.int16)[:, 24:30] = 20
        self.agent_buf[:, 62] = 1 << 2  # u16 pack: time_int_steps code 0 (= 2), active_block 1
        self._open(L.Config(dev.index or 0, N, T, mode, int(select_and_place), int(size_reward), self.max_steps,
                            int(autoreset), float(right_placement_scale), float(wrong_placement_scale),
                            int(lanes_per_env), int(debug_flags), int(env_index_base)),
                   z((L.STAT_STRIPES, 8), torch.int64))
        self.user_target = None
        self._have_tasks = False
        self._tasks_filled = 0       # rows of the task table written so far (what task sampling draws from)
        self._sampling = None        # (seed,) / ('random', kwargs) of the device-side generator, for sub-batches
        self._traj = None
        self._children = []
        # bumped by every call that changes what a step LAUNCH is given by value (the kernel parameters: sampler
        # settings, the episode-log buffers): a captured StepGraph carries the values of its capture
        self.config_epoch = 0
        self.render_size = (int(render_size[0]), int(render_size[1]))
        self._render_atlas = None
        # what reset / step draw (renderer='hip'): the persistent tensors of pov_outputs; pov is obs['pov'], [N, H, W, 3]
        self.pov_outputs = pov_outputs if renderer == 'hip' else ()
        pov = None
        if renderer == 'hip' and pov_obs is None:
            pov = _Pov(R.targets(N, self.render_size, 3, pov_outputs, None, dev)[0])
        elif renderer == 'hip':   # the stack, and the frame unless pov_frame=False: one igw_render_pov_obs launch
            W, H = self.render_size
            frame = {'rgb': R.targets(N, self.render_size, 3, None, None, dev)[0]} if pov_frame else {}
            pov = _Pov(frame, pov_obs, torch.zeros(pov_obs.shape(N, (W, H)), dtype=pov_obs.dtype, device=dev))
        self.pov_obs_spec = pov_obs
        self._fill = _FillFlag(N, dev)   # raised: the first draw fills
        if action_mask:
            Q.load()   # (built before the first step, not inside it)
        goal = ('todo',) if goal is True else tuple(goal or ())
        if [k for k in goal if k not in ('want', 'todo', 'gain')]:
            raise ValueError(f"goal names 'want', 'todo' and / or 'gain', got {goal!r}")
        if 'gain' in goal:
            QR.check_gain(mode != L.WALKING_DISCRETE, size_reward)
            Q.load()
        held = None
        if goal:
            G.load()
            held = G.outputs(N, ('align', 'fit') + tuple(k for k in ('want', 'todo') if k in goal) +
                             (('gain', 'ends') if 'gain' in goal else ()), dev)
        # obs['action_mask'] (action_mask=True): rewritten by every reset / step, and by whatever else moves the state
        self.vox_obs_spec = vox_obs
        vox = None
        if vox_obs is not None:
            X.load()
            vox = (vox_obs, torch.zeros(vox_obs.shape(N), dtype=vox_obs.dtype, device=dev))
        self._follow_with(pov, z((N, Q.ACTIONS), torch.uint8) if action_mask else None, held, vox)

    def _make_views(self):
        """The observation / result tensors of the env protocol (env.py:281-303) and the per-env task row / episode
        counter as strided VIEWS of the records the kernels read and write (include/igw.h): nothing is copied.
        They are NOT dense [N] tensors: agent_pos [N,5], inventory [N,6], compass [N], reward [N] are float32 views
        with a row stride of 16 elements (the 64-byte output record), done [N] is uint8 with stride 64, env_task /
        episode int32 with stride 4, grid [N,9,11,11] int8 with row stride 1104.  A consumer that needs packed
        memory (.view(), DLPack, a custom kernel indexing [i]) takes `dense()` or calls .contiguous().
        The first-person frame (renderer='hip', render_pov) is rendered from this same state, so it follows the same
        convention as `grid`: after a step that ended an episode of an auto-reset env, the frame shows the NEW
        episode's first state (the pose and grid the reset wrote), not the last state of the finished one."""
        N = self.num_envs
        f = self.out_buf.view(torch.float32)          # [N, 16]
        self.agent_pos = f[:, 0:5]                    # x, y, z, pitch, yaw
        self.inventory = f[:, 5:11]
        self.compass = f[:, 11]
        self.reward = f[:, 12]
        self.done = self.out_buf[:, 52]
        a = self.aux_buf.view(torch.int32)            # [N, 4]
        self.env_task = a[:, 2]                       # row of the task table
        self.episode = a[:, 3]                        # episodes started (keys the device-side task generators)
        self.grid = torch.as_strided(self.grid_buf, (N, 9, 11, 11), (L.GRID_STRIDE, 121, 11, 1))
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()

    # ---- tasks (GridWorld.set_task / Task.__init__ / initialize_world) ----
    def set_tasks(self, targets, starts=None, full_grids=None, invariant=None, init_pose=None,
                  env_task=None, first=0):
        """Fills task-table rows [first, first+T).  targets/starts/full_grids: dense [T,9,11,11];
        invariant: bool or [T]; init_pose: [T,5] (x,y,z,yaw,pitch).  Does not reset."""
        dev = self.device
        tgt = _as_rows(targets, dev)
        T = tgt.shape[0]
        st = _as_rows(starts, dev)
        fg = _as_rows(full_grids, dev)
        inv = _invariant(invariant, T, dev)
        for name, g, hi in (('targets', tgt, 7), ('starts', st, 6), ('full_grids', fg, 7)):
            # block ids are 0..7 (the observation space's range, env.py:85); a starting block is taken off the inventory
            # of its colour, ids 1..6 (env.py:243-246: the reference raises IndexError for 7).  The C ABI counts
            # offending rows (IGW_STAT_BAD_TASK) and reads such a cell as empty.
            if g is not None and g.numel() and (int(g.min()) < 0 or int(g.max()) > hi):
                raise ValueError(f'{name}: block ids must be in 0..{hi}')
        if first < 0 or first + T > self.num_tasks:
            raise ValueError(f'task rows [{first}, {first + T}) do not fit the table of {self.num_tasks}')
        for name, g in (('starts', st), ('full_grids', fg)):
            if g is not None and g.shape[0] != T:
                raise ValueError(f'{name} has {g.shape[0]} rows, targets {T}')
        pose = None
        if init_pose is not None:
            pose_np = np.asarray(init_pose, dtype=np.float64).reshape(T, 5)
            # the kernels index the world around the agent without range checks; that holds for |x|, |z| <= 10
            # (the C ABI replaces anything else by the default pose and counts it, IGW_STAT_BAD_POSE)
            ok = np.isfinite(pose_np).all() and (np.abs(pose_np[:, [0, 2]]) <= 10).all() and \
                (np.abs(pose_np[:, 1]) <= 64).all() and (np.abs(pose_np[:, 3:]) <= 1e6).all()
            if not ok:
                raise ValueError('init_pose must be finite with |x|, |z| <= 10, |y| <= 64 and |yaw|, |pitch| <= 1e6')
            pose = torch.as_tensor(pose_np, device=dev).contiguous()
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        L.check(self.lib.igw_prepare_tasks(self.ctx, first, T, ptr(tgt), ptr(st), ptr(fg), ptr(inv), ptr(pose),
                                           self._stream()), 'igw_prepare_tasks')
        if self.user_target is None:
            self.user_target = torch.zeros((self.num_tasks, L.GRID_STRIDE), dtype=torch.int8, device=dev)
        self.user_target[first:first + T] = tgt
        self._tasks_filled = max(self._tasks_filled, first + T)
        if env_task is not None:
            et = np.asarray(env_task.cpu() if torch.is_tensor(env_task) else env_task).reshape(-1)
            if et.shape[0] != self.num_envs or et.min() < 0 or et.max() >= self.num_tasks:
                raise ValueError(f'env_task needs {self.num_envs} indices into the task table [0, {self.num_tasks})')
            self.env_task.copy_(torch.as_tensor(et.astype(np.int32), device=dev))
        elif first == 0:
            if T == self.num_envs:
                self.env_task.copy_(torch.arange(self.num_envs, dtype=torch.int32, device=dev))
            elif T == 1:
                self.env_task.zero_()
        self._keep = (tgt, st, fg, inv, pose)  # keep inputs alive until the async kernel ran
        self._have_tasks = True
        self._fill.raise_()   # (the episode boundaries may have moved; nothing is drawn and the state is as it was)

    def set_task_sampling(self, enabled=True, seed=0, n_tasks=None):
        """Draw every env's task uniformly from the filled rows of the task table at each reset / auto-reset, on
        the device (CustomTasks.reset semantics; counter RNG keyed by seed, global env index and the env's
        episode counter, so it also advances inside a replayed HIP graph)."""
        n = int(n_tasks if n_tasks is not None else self._tasks_filled)
        if enabled and not 0 < n <= self.num_tasks:
            raise ValueError('set_task_sampling needs filled task rows: call set_tasks first')
        L.check(self.lib.igw_set_task_sampling(self.ctx, int(bool(enabled)), int(seed), n), 'igw_set_task_sampling')
        self._sampling = ('table', int(seed), n) if enabled else None
        self.config_epoch += 1
        for c in self._children:
            c._inherit_sampling()

    def set_random_tasks(self, enabled=True, seed=0, max_blocks=4, height_levels=1, max_dist=2, num_colors=1):
        """RandomTasks(max_blocks, height_levels, max_dist=.., num_colors=..) (gridworld/tasks/task_set.py:59-157)
        with sample_task() on the device: every reset / auto-reset writes a freshly sampled target into the env's
        own task row -- no host in the reset path.  Needs num_tasks == num_envs (the default)."""
        kw = dict(max_blocks=int(max_blocks), height_levels=int(height_levels), max_dist=int(max_dist),
                  num_colors=int(num_colors))
        L.check(self.lib.igw_set_random_tasks(self.ctx, int(bool(enabled)), int(seed), kw['max_blocks'],
                                              kw['height_levels'], kw['max_dist'], kw['num_colors'], self._stream()),
                'igw_set_random_tasks')
        self._sampling = ('random', int(seed), kw) if enabled else None
        self.config_epoch += 1
        if enabled:
            self._have_tasks = True
            self._tasks_filled = max(self._tasks_filled, self.num_envs)
        for c in self._children:
            c._inherit_sampling()

    def targets(self):
        """Current synthetic target (target - start) of every env, [N, 9, 11, 11] int8 (a gather from the task table)."""
        rows = self.task_target[self.env_task.long()]
        return rows[:, :L.CELLS].reshape(self.num_envs, 9, 11, 11)

    # ---- episode log (the reference's Logged wrapper, gridworld/wrappers.py:66-134, without video) ----
    def enable_trajectory_log(self, n_envs=1, capacity=None):
        """The first n_envs envs record every step on the device (one 64-byte record per step, two episode slots
        per env); see gridworld_amd.wrappers.EpisodeLogger for the npz dumps."""
        n_envs = int(n_envs)
        cap = int(capacity or self.max_steps)
        rec = torch.zeros((n_envs, 2, cap, L.TRAJ_BYTES), dtype=torch.uint8, device=self.device)
        heads = torch.zeros((n_envs, 2, 4), dtype=torch.int32, device=self.device)
        L.check(self.lib.igw_set_trajectory_log(self.ctx, rec.data_ptr(), heads.data_ptr(), n_envs, cap),
                'igw_set_trajectory_log')
        self._traj = (rec, heads, n_envs, cap)
        self.config_epoch += 1
        return rec, heads

    def disable_trajectory_log(self):
        L.check(self.lib.igw_set_trajectory_log(self.ctx, None, None, 0, 0), 'igw_set_trajectory_log')
        self._traj = None
        self.config_epoch += 1

    _STATE_KEYS = ('grid_buf', 'occ_buf', 'hist_buf', 'agent_buf', 'aux_buf', 'out_buf', 'task_target', 'task_start',
                   'task_start_occ', 'task_meta', 'task_index', 'stats_buf')

    def state_dict(self):
        """Snapshot of the complete env state (tensors are cloned): resume / parity debugging."""
        d = {k: getattr(self, k).clone() for k in self._STATE_KEYS}
        d['abi_version'] = L.VERSION
        return d

    def load_state_dict(self, state):
        """Restores a state_dict() snapshot.  The key set must be complete and of this ABI version: the step kernels
        read every one of these buffers (a snapshot without the colour index, say, would load and then drift)."""
        if state.get('abi_version') != L.VERSION:
            raise ValueError(f'state_dict is of ABI version {state.get("abi_version")!r}, this build is version {L.VERSION}')
        missing = [k for k in self._STATE_KEYS if k not in state]
        extra = [k for k in state if k not in self._STATE_KEYS and k != 'abi_version']
        if missing or extra:
            raise ValueError(f'state_dict keys do not match: missing {missing}, unexpected {extra}')
        for k in self._STATE_KEYS:
            if tuple(state[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f'state_dict[{k!r}] has shape {tuple(state[k].shape)}, expected {tuple(getattr(self, k).shape)}')
        for k in self._STATE_KEYS:
            getattr(self, k).copy_(state[k])
        self._have_tasks = True
        self._follow(draw=False)

    # ---- reset / step ----
    def _need_tasks(self):
        if not self._have_tasks:
            raise ValueError('Task is not initialized! Initialize task before working with the environment '
                             'using .set_tasks')

    def dense(self):
        """Packed COPIES of the per-step results for consumers that cannot take strided views (see _make_views):
        dict(agentPos [N,5], inventory [N,6], compass [N], reward [N], done [N] uint8), each contiguous."""
        return {'agentPos': self.agent_pos.contiguous(), 'inventory': self.inventory.contiguous(),
                'compass': self.compass.contiguous(), 'reward': self.reward.contiguous(), 'done': self.done.contiguous()}

    def reset(self, mask=None, keep_size=False):
        self._need_tasks()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        L.check(self.lib.igw_reset(self.ctx, None if m is None else C.c_void_p(m.data_ptr()),
                                   L.RESET_KEEP_SIZE if keep_size else 0, self._stream()), 'igw_reset')
        self._mask_keep = m
        self._follow(None if m is None else m.reshape(-1), fill=m is None)
        return self.obs()

    @staticmethod
    def _check_camera(cam):
        """Host-side mirror of the kernels' camera screen (IGW_CAMERA_MAX): camera deltas that arrive as HOST data
        are checked here and raise; device tensors are not read back (that would synchronise every step) -- the
        kernels run an offending component as a no-op and count it in stats()['bad_actions']."""
        if torch.is_tensor(cam):
            if cam.is_cuda:
                return
            c = cam.detach().numpy()
        else:
            c = np.asarray(cam)
        c = c.astype(np.float64, copy=False)
        if c.size and not (np.isfinite(c).all() and np.abs(c).max() <= L.CAMERA_MAX):
            raise ValueError(f'camera deltas must be finite with |value| <= {L.CAMERA_MAX:g} degrees')

    def step(self, actions):
        """walking: int32 tensor [N]; walking with discretize=False: dict(buttons u8[N,8] = forward, back,
        left, right, jump, attack, use, hotbar -- or those eight keys separately -- and camera f32[N,2]);
        flying: dict(movement f32[N,3], camera f32[N,2], inventory i32[N], placement i32[N]).
        Returns (obs, reward, done, info) of tensors living in HBM -- STRIDED views of the kernels' 64-byte output
        record (reward: float32, stride 16 elements; done: uint8, stride 64; see _make_views / dense()), the same
        tensors every call.  Actions that already are contiguous device tensors of the kernel's dtypes (walking: int32
        [N]; flying: float32 / int32) go straight to the C ABI: no conversion, no copy, one ctypes call."""
        if not self._have_tasks:
            self._need_tasks()
        bufs = self._action_buffers(actions)
        sp = self._space
        rc = getattr(self.lib, sp.step)(self.ctx, *[b.data_ptr() for b in bufs],
                                         torch._C._cuda_getCurrentRawStream(self._dev_index))
        if rc:
            L.check(rc, sp.step)
        self._act_keep = bufs   # the launch reads them asynchronously
        self._follow(self._ended())
        return self._obs.copy(), self.reward, self.done, {}

    def _action_buffers(self, actions, steps=None):
        """The action buffers of the env's space (_SPACES) as the entries take them: contiguous device tensors of the
        kernel's dtypes, for one step (steps=None; any shape of N rows) or as [T, N, ...] sequences (steps = who asks).
        A tensor that already is one is passed on as it is; anything else is converted -- except for
        steps='capture_steps', whose graph reads the caller's buffers at replay time: ValueError."""
        sp, N, dev, bufs = self._space, self.num_envs, self.device, []
        for (key, dt, shape), count in zip(sp.buffers, sp.counts):
            if key is None:
                x = actions
            elif key == 'buttons' and steps is None and 'buttons' not in actions:   # the reference's keys, one array each
                x = torch.stack([torch.as_tensor(np.asarray(actions[k]), device=dev).to(dt).reshape(-1)
                                 for k in BUTTONS], dim=1)
            else:
                x = actions[key]
            if not (type(x) is torch.Tensor and x.dtype is dt and x.is_cuda and x.is_contiguous()):
                if steps == 'capture_steps':
                    raise ValueError(f'capture_steps: {key or "actions"} must be a contiguous {dt} device tensor '
                                     f'[T, {", ".join(map(str, (N, *shape)))}]')
                if key == 'camera':   # (host data only: _check_camera does not read a device tensor back)
                    self._check_camera(x)
                x = torch.as_tensor(x, device=dev).to(dt).contiguous()
            if steps is None:
                ok = x.numel() == N * count
            else:
                ok = tuple(x.shape[1:]) == (N, *shape) and x.dim() == 2 + len(shape) and \
                    (not bufs or x.shape[0] == bufs[0].shape[0])
            if not ok:
                raise sp.mismatch(steps or 'step', N, key, x, 'T' if steps else '')
            bufs.append(x)
        return bufs

    # ---- first-person frames (libigw_render.so, include/igw_render.h) ----
    def render_pov_obs(self, spec, out=None, restart=None, fill=False, frame=None):
        """The observation of every env's CURRENT state in the layout `spec` (a render.ObsSpec or a dict), for callers
        who keep their own stack: one igw_render_pov_obs launch on the current stream that shifts this frame into `out`
        (the [N, K * planes, H, W] tensor of spec.dtype an earlier call returned), restarting the stack of env i where
        `restart` (a uint8 / bool device tensor [N], any stride) is not 0, of every env with fill=True.  out=None
        returns a new, filled tensor; with `out` nothing is allocated, so the call can be captured.  `frame` (uint8
        [N, H, W, 3]) also receives what render_pov() draws."""
        spec = R.ObsSpec.of(spec)
        if restart is not None and not (torch.is_tensor(restart) and restart.dtype in (torch.uint8, torch.bool)):
            restart = torch.as_tensor(restart, device=self.device).ne(0).to(torch.uint8)
        return _render_obs_rows(self, spec, out, frame, restart, fill, self._stream())

    def set_render_atlas(self, atlas):
        """The texture atlas of render_pov: uint8 [S, S, 4] (numpy or tensor, row 0 = the top image row), S a multiple
        of 8 up to 256 -- e.g. render.load_atlas('texture.png') of the reference for its look.  Default: the flat-colour
        atlas of render.default_atlas()."""
        self._render_atlas = R.device_atlas(atlas, self.device)

    def render_views(self, poses, rows=None, what='grid', **kw):
        """Views of the batch from cameras of the caller's choice (visualizer.render_views): uint8 [M, H, W, channels]
        for poses [M, 5] float64 (x, y, z, yaw, pitch).  what='grid': the envs' CURRENT grids, read in place from
        grid_buf, `rows` = the env of each view (the spectator camera); what='target' / 'start': the target / starting
        grid of task-table rows, `rows` = the task row of each view (the goal image; env_task maps envs to rows; the
        table's target is the one the reward counts: the task's target grid, less its starting grid if it has one).
        rows=None: view v shows row v.  One launch on the current stream, with the env's atlas and render_size unless
        `atlas` / `size` say otherwise; `channels`, `out`, `outputs`, `codec` and `quality` as for render_pov.  It keeps
        no frame tensor, so it needs no renderer='hip' at construction."""
        from . import visualizer as V
        try:
            grids = {'grid': self.grid_buf, 'target': self.task_target, 'start': self.task_start}[what]
        except KeyError:
            raise ValueError(f"what must be 'grid', 'target' or 'start', got {what!r}") from None
        kw.setdefault('size', self.render_size)
        if kw.get('atlas') is None:
            kw['atlas'] = self._atlas()
        return V.render_views(grids, poses, view_grid=rows, device=self.device, **kw)

    # ---- a captured step loop (the loop of examples/run_env.py:18-26 as ONE HIP-graph launch) ----
    def capture_steps(self, actions, record=False, chains=1):
        """Captures `for t in range(T): env.step(actions[t])` into a HIP graph and returns a StepGraph; replay() launches
        the T steps in one call (no per-step host work at all), bit-identical to the eager loop.  chains = P > 1 captures
        the T steps as P INDEPENDENT chains of launches, one per contiguous sub-batch of N / P envs (envs never read one
        another's state, so the results are the same bytes), each a linear graph replayed on its own stream: the tail
        of one sub-batch's step t -- the wait for its slowest wavefront -- and the ramp of its step t + 1 can overlap the
        other sub-batches' work instead of idling the chip between two whole-batch launches (all action spaces; not
        with the episode log or the RandomTasks generator, which index by context).  `actions`: walking int32
        device tensor [T, N]; flying dict of device tensors movement f32[T,N,3], camera f32[T,N,2], inventory i32[T,N],
        placement i32[T,N]; walking Dict: buttons u8[T,N,8], camera f32[T,N,2].  The graph reads the action BUFFERS at
        replay time: refill them in place (copy_) between replays to step with new actions.  record=True also copies
        every step's output record (StepGraph.outs uint8 [T, N, 64]; .rewards / .dones are views of it).  What varies
        between replays -- actions, env state, task table, the samplers' episode counters, the log's heads -- lives in
        device memory (include/igw.h), so samplers, auto-resets and the episode log advance inside the replayed graph
        exactly as they do eagerly.  What does NOT: the sampler SETTINGS and the episode-log buffers are kernel
        parameters, frozen at capture; after set_task_sampling / set_random_tasks / enable_ / disable_trajectory_log
        replay() raises (capture again).  With renderer='hip' the graph ends with the launch that draws obs['pov'] (and
        the planes of pov_outputs) of the state after the last step: what the eager loop's last step() leaves there.
        With a pov_obs of stack > 1 the draw follows EVERY step launch of its chain inside the graph (each frame has to
        enter the stack), with the eager loop's restart rule; replay() returns obs['pov_obs'] too."""
        self._need_tasks()
        return StepGraph(self, actions, record, chains)

    def _before_capture(self):
        """What _follow_captured reads and a capture may not allocate."""
        if self._pov is not None:
            self._atlas()
        if (self._pov is not None and self._pov.stacked) or (self._vox is not None and self._vox[0].stack > 1):
            self._fill.on_device(self)

    def _replayed(self, chains):
        """What StepGraph.replay returns, step()'s result; the first draws of the graph's `chains` (its sub-batches, if
        it has any) took the stacks' fill flags."""
        if self.pov_obs is not None or self._vox is not None:
            self._fill.lowered(self, *chains)
        return self._obs.copy(), self.reward, self.done, {}

    def rollout(self, T, seed, t0=0, env_offset=0):
        """T fused walking steps per env with counter-RNG actions and auto-reset (one launch)."""
        self._need_tasks()
        L.check(self.lib.igw_rollout_walking(self.ctx, int(T), int(seed), int(t0), int(env_offset),
                                             self._stream()), 'igw_rollout_walking')
        self._follow(draw=False)

    def rollout_actions(self, actions, return_rewards=False):
        """Fused replay of a recorded action sequence: `actions` int32 [T, N] (Discrete(18) ids), or for the flying action
        space a dict of [T, N, ...] arrays (movement, camera, inventory, placement) -- bit-identical to
        T calls of step(), in one launch without a barrier between the steps of different envs (the context's
        autoreset setting applies).  With return_rewards: (rewards float32 [T, N], dones uint8 [T, N])."""
        self._need_tasks()
        N, dev, sp = self.num_envs, self.device, self._space
        if sp.rollout is None:
            raise L.IgwError('rollout_actions: Discrete(18) walking and flying only')
        if self._traj is not None:
            raise L.IgwError('rollout / rollout_actions do not write the episode log: disable_trajectory_log() first')
        bufs = self._action_buffers(actions, 'rollout_actions')
        T = int(bufs[0].shape[0])
        rw = dn = None
        if return_rewards:
            rw = torch.empty((T, N), dtype=torch.float32, device=dev)
            dn = torch.empty((T, N), dtype=torch.uint8, device=dev)
        rp, dp = (rw.data_ptr() if rw is not None else None), (dn.data_ptr() if dn is not None else None)
        L.check(getattr(self.lib, sp.rollout)(self.ctx, *[b.data_ptr() for b in bufs], T, rp, dp, self._stream()),
                sp.rollout)
        self._keep = bufs  # the launch reads them asynchronously
        self._follow(draw=False)
        return (rw, dn) if return_rewards else None

    def fill_actions(self, n_steps, seed, t0=0, env_offset=0):
        a = torch.empty((n_steps, self.num_envs), dtype=torch.int32, device=self.device)
        L.check(self.lib.igw_fill_actions_walking(self.ctx, a.data_ptr(), int(n_steps), int(t0), int(seed),
                                                  int(env_offset), self._stream()), 'igw_fill_actions_walking')
        return a

    # ---- asynchronous sub-batches ----
    def split(self, parts, streams=None):
        """`parts` contiguous sub-batches that SHARE this env's tensors (each is a view of rows
        [lo, hi)) but have their own context and HIP stream, so they can be stepped independently --
        e.g. policy inference on one half overlaps env stepping of the other (EnvPool-style async mode).
        Envs are independent, so results are identical to stepping the whole batch.  Every sub-batch stream
        first waits for the work already queued on the current stream (set_tasks / reset / steps of the parent);
        SubBatch.synchronize() / join() order the current stream after the sub-batch again."""
        if self.num_envs % parts:
            raise ValueError('num_envs must be divisible by parts')
        n = self.num_envs // parts
        streams = streams or [torch.cuda.Stream(device=self.device) for _ in range(parts)]
        cur = torch.cuda.current_stream(self.device)
        subs = []
        for k in range(parts):
            streams[k].wait_stream(cur)
            subs.append(SubBatch(self, k * n, n, streams[k]))
        self._children.extend(subs)
        return subs

    def _release_children(self, subs):
        """Sub-batches that are no longer needed: their counters move into this env's own buffer."""
        for c in subs:
            if c in self._children:
                self.stats_buf += c.stats_buf
                self._children.remove(c)

    # ---- introspection ----
    def stats_tensor(self):
        """The device counters [8] int64 of this env and its sub-batches as a DEVICE tensor (no synchronisation)."""
        s = self.stats_buf.sum(0)
        for c in self._children:
            s = s + c.stats_buf.sum(0)
        return s

    def stats(self):
        """Device counters of this env and of its sub-batches (VecGridWorld.split).  `steps`: env-steps executed, counted
        on the device by every step launch and fused rollout (`rollout_steps` is the same counter's old name)."""
        s = self.stats_tensor().cpu()
        return {'changed': int(s[L.STAT_CHANGED]), 'resets': int(s[L.STAT_RESETS]),
                'steps': int(s[L.STAT_STEPS]), 'rollout_steps': int(s[L.STAT_STEPS]), 'rescans': int(s[L.STAT_RESCANS]),
                'bad_poses': int(s[L.STAT_BAD_POSE]), 'bad_actions': int(s[L.STAT_BAD_ACTION]),
                'bad_tasks': int(s[L.STAT_BAD_TASK])}

    def internals(self):
        """float64 [N,8]: x, y, z, yaw, pitch, dy, time_int_steps, active_block (debug / parity)."""
        raw = self.agent_buf.cpu().numpy()
        out = np.zeros((self.num_envs, 8), np.float64)
        out[:, :6] = raw[:, :48].copy().view(np.float64)
        pack = raw[:, 62:64].copy().view(np.uint16)[:, 0].astype(np.int64)
        out[:, 6] = np.array([2, 4, 8, 12])[pack & 3]
        out[:, 7] = (pack >> 2) & 7
        return out

    def task_state(self):
        raw, aux = self.agent_buf.cpu().numpy(), self.aux_buf.cpu().numpy()
        i16 = aux[:, :8].copy().view(np.int16).astype(np.int64)
        return {'step_no': raw[:, 60:62].copy().view(np.uint16)[:, 0].astype(np.int64),
                'inventory': raw[:, 48:60].copy().view(np.int16).astype(np.int64),
                'size': i16[:, 0], 'prev_size': i16[:, 1] & 0x7fff, 'dirty': (i16[:, 1] >> 15) & 1,
                'max_int': i16[:, 2], 'target_size': i16[:, 3]}

    def set_step_no(self, step_no):
        """Overwrites GridWorld.step_no of every env (int tensor / array [N]): de-synchronises the episodes of a batch."""
        sn = torch.as_tensor(step_no).to(device=self.agent_buf.device, dtype=torch.int16).reshape(self.num_envs)
        self.agent_buf.view(torch.int16)[:, 30] = sn


class StepGraph:
    """T captured env steps (VecGridWorld.capture_steps).  replay() launches them on the current stream and returns the
    env's (obs, reward, done, info) views, which then hold the LAST step's values."""

    def __init__(self, env, actions, record, chains=1):
        self.env = env
        dev, N = env.device, env.num_envs
        chains = int(chains)
        if chains < 1 or N % chains:
            raise ValueError(f'capture_steps: chains must divide num_envs ({N})')
        if chains > 1 and (env._traj is not None or (env._sampling or ('',))[0] == 'random'):
            raise L.IgwError('capture_steps(chains > 1) cannot be combined with the episode log or the RandomTasks generator')
        self.chains = chains
        # A launch is given the kernel parameters BY VALUE: the graph freezes the sampler settings (set_task_sampling,
        # set_random_tasks) and the episode-log buffers (enable / disable_trajectory_log) of the moment of capture.
        # replay() refuses to run after any of them changed (config_epoch), and the graph keeps the log's buffers
        # alive, so a stale graph can neither run a stale configuration silently nor write into freed memory.
        self.config_epoch = env.config_epoch
        self._held = env._traj
        self.buffers = tuple(env._action_buffers(actions, 'capture_steps'))   # (validated; never converted)
        self.T = T = int(self.buffers[0].shape[0])
        if T < 1:
            raise ValueError('capture_steps: every action buffer needs the same number of steps T >= 1')
        self.outs = torch.zeros((T, N, L.OUT_BYTES), dtype=torch.uint8, device=dev) if record else None
        fn, row_bytes = getattr(env.lib, env._space.step), env._space.row_bytes
        self.graph = torch.cuda.CUDAGraph()
        cur = torch.cuda.current_stream(dev)
        # (thread-local: other threads of the process -- an RCCL watchdog, a data loader -- may touch the runtime)
        # chains > 1: one context, one stream and ONE LINEAR GRAPH per chain, replayed side by side on their streams.
        # (Measured, profiles/r05_chains.txt: captured as parallel BRANCHES of one graph the chains do not overlap --
        # the runtime executes the branches one after the other, 2 / 4 / 8 branches cost 12.3 / 16.6 / 25.6 us per
        # step against 10.9 for the single chain -- while kernels of different STREAMS do run concurrently.)
        self.subs = env.split(chains) if chains > 1 else None   # (kept alive with the graphs)
        self.graphs = [self.graph] + [torch.cuda.CUDAGraph() for _ in range(chains - 1)]
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(chains)]
        env._before_capture()
        for part, graph, st in zip(self.subs or [env], self.graphs, self.streams):
            st.wait_stream(cur)
            lo, n = part.lo, part.num_envs
            ptrs = [[b[t].data_ptr() + lo * rb for b, rb in zip(self.buffers, row_bytes)] for t in range(T)]
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                h = C.c_void_p(st.cuda_stream)
                for t in range(T):
                    L.check(fn(part.ctx, *ptrs[t], h), 'step (capture)')
                    if record:
                        self.outs[t, lo:lo + n].copy_(env.out_buf[lo:lo + n])
                    part._follow_captured(h, t == 0, t == T - 1)
            cur.wait_stream(st)
        if record:
            f = self.outs.view(torch.float32)
            self.rewards, self.dones = f[:, :, 12], self.outs[:, :, 52]

    def __del__(self):
        # the chains' contexts were registered with the env for its counters: fold their counts into the env's own
        # buffer and let them go (a bench that captures many graphs must not accumulate contexts)
        subs, env = getattr(self, 'subs', None), getattr(self, 'env', None)
        if subs and env is not None:
            try:
                env._release_children(subs)
            except Exception:  # noqa: BLE001 -- interpreter shutdown
                pass

    def replay(self):
        env = self.env
        if env.config_epoch != self.config_epoch:
            raise L.IgwError('StepGraph is stale: set_task_sampling / set_random_tasks / enable_trajectory_log / '
                             'disable_trajectory_log was called after capture_steps (a captured launch carries those '
                             'settings by value); capture the steps again')
        if self.chains == 1:
            self.graph.replay()
        else:   # fork: every chain's stream waits for the caller's stream, runs its graph; the caller's stream joins
            cur = torch.cuda.current_stream(env.device)
            for g, st in zip(self.graphs, self.streams):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    g.replay()
            for st in self.streams:
                cur.wait_stream(st)
        return env._replayed(self.subs or ())


class SubBatch(_Rows):
    """Rows [lo, lo + n) of a VecGridWorld behind their own igw context and stream (VecGridWorld.split).
    The context carries the parent's global env offset, so device-side task generators draw the streams the
    whole batch would draw, and inherits the parent's generator settings."""
    _SHARED = ('lib', 'device', 'render_size', 'pov_outputs', 'autoreset', 'flying', 'walk_dict', 'select_and_place')
    _VIEWS = ('agent_pos', 'inventory', 'compass', 'reward', 'done', 'grid')   # VecGridWorld._make_views

    def __init__(self, parent, lo, n, stream):
        self.parent, self.lo, self.stream = parent, lo, stream
        for k in self._SHARED:
            setattr(self, k, getattr(parent, k))
        cfg = L.Config.from_buffer_copy(parent.cfg)
        cfg.num_envs = n
        cfg.env_index_base = parent.env_index_base + lo
        if cfg.lanes_per_env == 0:   # the group width the library chose for the WHOLE batch (include/igw.h: IGW_AUTO_*)
            cfg.lanes_per_env = L.auto_lanes(parent.num_envs)
        self._open(cfg, torch.zeros_like(parent.stats_buf))
        sl = self._sl
        for k in self._VIEWS:
            setattr(self, k, getattr(parent, k)[sl])
        self._follow_with(parent._pov and parent._pov.rows(sl), None if parent._mask is None else parent._mask[sl],
                          None if parent._goal is None else {k: t[sl] for k, t in parent._goal.items()},
                          None if parent._vox is None else (parent._vox[0], parent._vox[1][sl]))
        if parent in parent._fill.drawn:   # (a sub-batch of a batch whose stacks are current starts with them)
            parent._fill.lowered(self)
        self._inherit_sampling()

    def _inherit_sampling(self):
        sp = self.parent._sampling
        if sp is None:
            L.check(self.lib.igw_set_task_sampling(self.ctx, 0, 0, 0), 'igw_set_task_sampling')
            L.check(self.lib.igw_set_random_tasks(self.ctx, 0, 0, 1, 1, 1, 1, None), 'igw_set_random_tasks')
        elif sp[0] == 'table':
            L.check(self.lib.igw_set_task_sampling(self.ctx, 1, sp[1], sp[2]), 'igw_set_task_sampling')
        else:  # generated rows are indexed by the context's local env, a sub-batch would overwrite rows of another
            raise L.IgwError('the RandomTasks generator cannot be combined with sub-batches')

    def reset(self):
        L.check(self.lib.igw_reset(self.ctx, None, 0, self._stream()), 'igw_reset')
        self._follow(fill=True)
        return self.obs()

    def synchronize(self):
        self.stream.synchronize()

    def join(self):
        """Orders the current stream after everything queued on this sub-batch (no host wait)."""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)


class _Pov:
    """The persistent outputs of renderer='hip': output name -> tensor as pov_outputs names them, for the whole batch
    or, through rows(), for a SubBatch's slice of the same memory (_Rows._draw draws them).  The default, ('rgb',), is
    drawn by the plain entry (render.launch with outputs=None); anything else by one _aux launch.  With pov_obs, `obs`
    is the stack tensor [N, K * planes, H, W] of `spec` and `tensors` holds the frame or nothing (pov_frame=False): one
    igw_render_pov_obs launch (render.launch_obs) draws both; `stacked` says that the stack holds more than the
    current frame, so that every frame has to enter it."""

    def __init__(self, tensors, spec=None, obs=None):
        self.tensors, self.spec, self.obs = tensors, spec, obs
        self.plain = tuple(tensors) == ('rgb',) and obs is None
        self.stacked = obs is not None and spec.stack > 1

    def rows(self, sl):
        return _Pov({k: t[sl] for k, t in self.tensors.items()}, self.spec, None if self.obs is None else self.obs[sl])

    def add_to(self, obs):
        """Adds the tensors to an observation dict, 'rgb' as 'pov', the planes under their names and the stack as
        'pov_obs'; returns it."""
        for k, t in self.tensors.items():
            obs['pov' if k == 'rgb' else k] = t
        if self.obs is not None:
            obs['pov_obs'] = self.obs
        return obs


finished_episodes = QR.finished_episodes   # (tools/ read it from here)


def _render_rows(env, out, channels, size, outputs, stream, alloc_stream=None):
    """One igw_render_pov launch (render.launch) over the state rows of a whole VecGridWorld or of a SubBatch."""
    agent, grid, occ = env._rows
    n = env.num_envs
    return R.launch('pov', (agent.data_ptr(), grid.data_ptr(), occ.data_ptr(), n), n,
                    size if size is not None else env.render_size, channels, outputs, out, env._atlas(), env.device,
                    stream, alloc_stream)


def _render_obs_rows(env, spec, out, frame, restart, fill, stream, alloc_stream=None):
    """One igw_render_pov_obs launch (render.launch_obs) over the state rows of a whole VecGridWorld or of a SubBatch."""
    agent, grid, occ = env._rows
    n = env.num_envs
    return R.launch_obs((agent.data_ptr(), grid.data_ptr(), occ.data_ptr(), n), n, env.render_size, spec, out, frame,
                        restart, fill, env._atlas(), env.device, stream, alloc_stream)


def task_eval(targets, grids, full_grids=None, invariant=None, device='cuda:0'):
    """Task(target, full_grid, invariant).maximal_intersection / argmax_intersection on `grid`
    for n pairs (tasks/task.py:121-161), on the GPU.  Returns numpy (max_int, argmax[n,3], target_size)."""
    if not torch.cuda.is_available():
        raise L.IgwError('task_eval needs a HIP device (no CPU fallback)')
    lib = L.load()
    dev = torch.device(device)
    t, g, f = _as_rows(targets, dev), _as_rows(grids, dev), _as_rows(full_grids, dev)
    n = t.shape[0]
    inv = _invariant(invariant, n, dev)
    mi = torch.zeros(n, dtype=torch.int32, device=dev)
    am = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    ts = torch.zeros(n, dtype=torch.int32, device=dev)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731
    L.check(lib.igw_task_eval(dev.index or 0, n, ptr(t), ptr(g), ptr(f), ptr(inv), ptr(mi), ptr(am), ptr(ts),
                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), 'igw_task_eval')
    return mi.cpu().numpy(), am.cpu().numpy(), ts.cpu().numpy()

"""The host side of the query libraries (goal, worth, aim, peek, peek_dict, relabel, recall, vox, query) without a device:
what each launch() accepts and rejects as `out`, what it allocates, and the pointer list it hands to its library entry.
Every launch runs on CPU tensors with the module's *_into function replaced by a recorder, so no library is loaded; the
tensors' geometry below is the documented one (each module's docstring and DESIGN.md sections 10 to 18), restated here.
The device side of the same calls is tests/test_gpu_*.py."""
import importlib

import pytest
import torch

CPU = torch.device('cpu')
ROW = 1104
GRID = (ROW, 121, 11, 1)          # the strides of a [.., 9, 11, 11] view of 1104-element rows


def _dense(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= max(s, 1)
    return tuple(reversed(st))


def _view(shape, strides, dtype, offset=0):
    """A zeroed tensor of that geometry cut from a larger buffer, `offset` elements behind a 64-byte boundary."""
    span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(shape) else 0
    base = torch.zeros(span + offset + 128, dtype=dtype)
    offset += (-base.data_ptr() % 64) // base.element_size()
    return torch.as_strided(base, shape, strides, offset)


def _never(*a, **kw):
    raise AssertionError('not to be reached')


class Case:
    """One query module: `outputs` in the library's order, name -> (shape, dtype, strides, alignment in bytes) of what a
    caller sees for n envs, the inputs of a launch, the launch itself and where the recorded call holds the pointers."""
    name = into = None
    outputs = ()
    n = 2
    zero = False                  # whether an allocation is zero-filled
    launches_empty = True         # whether the library entry is called for n = 0
    keyed = True                  # whether `out` is a dict (an unknown key can be given)

    @property
    def mod(self):
        return importlib.import_module('gridworld_amd.' + self.name)

    def subsets(self):
        return [self.outputs] + [(k,) for k in self.outputs]

    def state(self, n, count):
        return [torch.zeros((n, 16), dtype=torch.uint8) for _ in range(count)]


class Goal(Case):
    name, into, zero = 'goal', 'goal_into', True
    outputs = ('align', 'fit', 'want', 'todo', 'gain', 'ends')

    def spec(self, n):
        grid = ((n, 9, 11, 11), torch.int8, GRID, 16)
        return {'align': ((n, 3), torch.int8, (4, 1), 4), 'fit': ((n, 4), torch.int16, (4, 1), 8), 'want': grid,
                'todo': grid, 'gain': ((n, 18), torch.float32, (18, 1), 4), 'ends': ((n, 18), torch.uint8, (18, 1), 1)}

    def inputs(self, n):
        return self.state(n, 8), torch.zeros((n, 18), dtype=torch.uint8), torch.zeros((n, 2), dtype=torch.int16)

    def launch(self, inputs, n, names, out):
        state, mask, look = inputs
        return self.mod.launch(state, n, (1.0, 0.1, 250, True), mask, look, names, out, CPU, None)

    def pointers(self, args):
        return list(args[8])


class Worth(Case):
    name, into = 'worth', 'worth_into'
    outputs = ('word', 'best')

    def spec(self, n):
        return {'word': ((n, 7, 9, 11, 11), torch.int16, (7 * ROW,) + GRID, 16), 'best': ((n, 4), torch.int32, (4, 1), 16)}

    def inputs(self, n):
        return self.state(n, 8)

    def launch(self, state, n, names, out):
        return self.mod.launch(state, n, (1.0, 0.1, 250), None, False, names, out, CPU, None)

    def pointers(self, args):
        return list(args[7:9])


class Aim(Case):
    name, into = 'aim', 'aim_into'
    outputs = ('place', 'break')

    def spec(self, n):
        return {k: ((n, 9, 11, 11), torch.int32, GRID, 16) for k in self.outputs}

    def inputs(self, n):
        return self.state(n, 2)

    def launch(self, inputs, n, names, out):
        agent, occ = inputs
        return self.mod.launch(agent, occ, n, 72, 'place' in names, 'break' in names, out, CPU, None)

    def pointers(self, args):
        return list(args[4:6])


class Peek(Case):
    name, into = 'peek', 'peek_into'
    outputs = ('reward', 'ends', 'change', 'pose', 'ret')
    K, H = 2, 3

    def spec(self, n):
        k, h = self.K, self.H
        geo = {'reward': ((n, k, h), torch.float32), 'ends': ((n, k), torch.int16), 'change': ((n, k, h), torch.int16),
               'pose': ((n, k, 5), torch.float32), 'ret': ((n, k), torch.float32)}
        return {key: (shape, dtype, _dense(shape), 1) for key, (shape, dtype) in geo.items()}

    def inputs(self, n):
        return self.state(n, 9), torch.zeros((self.K, self.H), dtype=torch.int32)

    def launch(self, inputs, n, names, out):
        state, actions = inputs
        return self.mod.launch(state, n, actions, (1.0, 0.1, 250, True), 1.0, names, out, CPU, None)

    def pointers(self, args):
        return list(args[11])


class PeekDict(Peek):
    name = 'peek_dict'

    def inputs(self, n):
        k, h = self.K, self.H
        return self.state(n, 9), dict(movement=torch.zeros((k, h, 3)), camera=torch.zeros((k, h, 2)),
                                      inventory=torch.zeros((k, h), dtype=torch.int32),
                                      placement=torch.zeros((k, h), dtype=torch.int32))

    def launch(self, inputs, n, names, out):
        state, actions = inputs
        res, bufs = self.mod.launch('flying', state, n, actions, (1.0, 0.1, 250, True), 1.0, names, out, CPU, None)
        assert [b.data_ptr() for b in bufs] == [t.data_ptr() for t in actions.values()]
        return res

    def pointers(self, args):
        return list(args[12])


class Relabel(Case):
    name, into, launches_empty = 'relabel', 'relabel_into', False
    outputs = ('reward', 'done', 'progress', 'end', 'ret', 'target_size', 'target')
    G, L = 2, 3

    def spec(self, e):
        g, l = self.G, self.L
        step, pair = ((e, g, l), (g * l, l, 1)), ((e, g), (g, 1))
        geo = {'reward': step + (torch.float32,), 'done': step + (torch.uint8,), 'progress': step + (torch.int16,),
               'end': pair + (torch.int32,), 'ret': pair + (torch.float32,), 'target_size': pair + (torch.int16,),
               'target': ((e, g, 9, 11, 11), (g * ROW,) + GRID, torch.int8)}
        return {k: (shape, dtype, strides, 16 if k == 'target' else 1) for k, (shape, strides, dtype) in geo.items()}

    def inputs(self, e):
        return (torch.zeros((max(e, 1), self.L, 64), dtype=torch.uint8), torch.zeros(e, dtype=torch.int64),
                torch.zeros(e, dtype=torch.int32), torch.zeros((e, ROW), dtype=torch.int8),
                torch.zeros((e, self.G), dtype=torch.int32))

    def launch(self, inputs, e, names, out):
        records, first, length, starts, at = inputs
        return self.mod.launch(records, first, length, starts, None, at, self.L, (1.0, 0.1, 250), 1.0, names, out, CPU, None)

    def pointers(self, args):
        return list(args[14])


class Recall(Case):
    name, into, launches_empty = 'recall', 'recall_into', False
    outputs = ('obs', 'next_obs', 'record', 'valid')

    def vox_spec(self):
        from gridworld_amd import vox
        return vox.VoxSpec(planes=(('grid', 'onehot'),), agent=True, dtype=torch.float16, stack=2)

    def spec(self, b):
        obs = (b, 2 * 7, 9, 11, 11)
        geo = {'obs': (obs, torch.float16, 1), 'next_obs': (obs, torch.float16, 1), 'record': ((b, 64), torch.uint8, 4),
               'valid': ((b,), torch.uint8, 1)}
        return {k: (shape, dtype, _dense(shape), al) for k, (shape, dtype, al) in geo.items()}

    def inputs(self, b):
        return (torch.zeros((1, 4, 64), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64),
                torch.zeros(1, dtype=torch.int32), torch.zeros((1, ROW), dtype=torch.int8),
                torch.zeros((1, 5), dtype=torch.float64), torch.zeros(b, dtype=torch.int32), torch.ones(b, dtype=torch.int32))

    def launch(self, inputs, b, names, out):
        records, first, length, starts, pose, episode, step = inputs
        return self.mod.launch(records, first, length, starts, pose, episode, step, self.vox_spec(), None, None, 4, names,
                               out, CPU, None)

    def pointers(self, args):
        return list(args[16])


class Vox(Case):
    name, into, keyed = 'vox', 'vox_into', False
    outputs = ('obs',)

    def vox_spec(self):
        return self.mod.VoxSpec(planes=(('grid', 'onehot'), ('target', 'occ')), agent=True, dtype=torch.float32, stack=2)

    def spec(self, n):
        shape = (n, 2 * 8, 9, 11, 11)
        return {'obs': (shape, torch.float32, _dense(shape), 1)}

    def subsets(self):
        return [self.outputs]

    def inputs(self, n):
        return self.state(n, 2)

    def launch(self, inputs, n, names, out):
        agent, aux = inputs
        sources = [(agent.data_ptr(), None, ROW, 0), (aux.data_ptr(), aux.data_ptr(), ROW, 1)]
        return {'obs': self.mod.launch(agent, aux, n, self.vox_spec(), sources, (out or {}).get('obs'), None, False, CPU, None)}

    def pointers(self, args):
        return [args[3].data]


class Query(Case):
    """The tuple form: the mask is always written, `look` and `actions` when asked for; `out` is a tuple in that order
    (None entries are allocated), so "a key the call does not write" is a tuple longer than what the call writes."""
    name, into = 'query', 'action_mask_into'
    outputs = ('mask', 'look', 'actions')

    def spec(self, n):
        return {'mask': ((n, 18), torch.uint8, (18, 1), 1), 'look': ((n, 2), torch.int16, (2, 1), 1),
                'actions': ((n,), torch.int32, (1,), 1)}

    def subsets(self):
        return [self.outputs, ('mask',), ('mask', 'look'), ('mask', 'actions')]

    def inputs(self, n):
        return self.state(n, 2)

    def launch(self, inputs, n, names, out):
        agent, occ = inputs
        given = None
        if out:
            given = tuple(out.get(k) for k in names) + tuple(t for k, t in out.items() if k not in names)
        res = self.mod.launch(agent, occ, n, True, given, 'look' in names, (1, 2) if 'actions' in names else None, 0, CPU,
                              None)
        res = res if isinstance(res, tuple) else (res,)
        assert len(res) == len(names)
        return dict(zip(names, res))

    def pointers(self, args):
        return list(args[4:7])


CASES = {c.name: c for c in (Goal(), Worth(), Aim(), Peek(), PeekDict(), Relabel(), Recall(), Vox(), Query())}
case_of = pytest.mark.parametrize('case', list(CASES.values()), ids=list(CASES))


def _run(case, monkeypatch, n, names, out=None, forbid=()):
    """One launch on the CPU: (the result's tensors of `names`, the recorded library calls).  `forbid` names torch
    functions that raise while it runs."""
    calls, inputs = [], case.inputs(n)
    with monkeypatch.context() as m:
        m.setattr(case.mod, case.into, lambda *a: calls.append(a))
        m.setattr(case.mod.BINDING, 'load', _never)
        for f in forbid:
            m.setattr(torch, f, _never)
        res = case.launch(inputs, n, tuple(names), out)
    assert len(calls) <= 1
    return {k: t for k, t in res.items() if k in names}, calls


def _as_documented(case, n, res):
    for k, t in res.items():
        shape, dtype, strides, align = case.spec(n)[k]
        assert tuple(t.shape) == shape and t.dtype == dtype and t.device == CPU, (case.name, k)
        assert t.data_ptr() % align == 0, (case.name, k)
        if all(shape):
            assert tuple(t.stride()) == strides, (case.name, k)


@case_of
def test_a_launch_allocates_the_documented_tensors_and_takes_them_back_as_out(case, monkeypatch):
    n = case.n
    for names in case.subsets():
        res, calls = _run(case, monkeypatch, n, names)
        assert list(res) == [k for k in case.outputs if k in names] and len(calls) == 1
        _as_documented(case, n, res)
        want = [res[k].data_ptr() if k in names else None for k in case.outputs]
        assert case.pointers(calls[0]) == want, (case.name, names)
        # the previous result as `out`: the same objects, the same pointers, and no tensor is made
        again, calls = _run(case, monkeypatch, n, names, dict(res), forbid=('empty', 'zeros', 'as_strided'))
        assert all(again[k] is res[k] for k in names) and list(again) == list(res)
        assert case.pointers(calls[0]) == want
        # a part of it: the rest is allocated
        if len(names) > 1:
            part, calls = _run(case, monkeypatch, n, names, {names[-1]: res[names[-1]]})
            assert part[names[-1]] is res[names[-1]] and all(part[k] is not res[k] for k in names[:-1])
            _as_documented(case, n, part)
            assert case.pointers(calls[0]) == [part[k].data_ptr() if k in names else None for k in case.outputs]


@case_of
def test_an_allocation_is_zero_filled_for_the_goal_query_alone(case, monkeypatch):
    res, _ = _run(case, monkeypatch, case.n, case.outputs, forbid=('empty',) if case.zero else ('zeros',))
    if case.zero:
        for k, t in res.items():
            shape, _, strides, _ = case.spec(case.n)[k]
            raw = torch.as_strided(t, (case.n, strides[0]), (strides[0], 1))     # the rows with their padding
            assert not bool(raw.any()), k


def _wrong(case, n, k):
    """why -> a tensor that differs from the documented out[k] in that one respect."""
    shape, dtype, strides, align = case.spec(n)[k]
    other = torch.float64 if dtype is not torch.float64 else torch.int8
    more = (shape[0] + 1,) + shape[1:]
    bad = {'dtype': _view(shape, strides, other), 'shape': _view(more, strides, dtype),
           'meta': torch.empty_strided(shape, strides, dtype=dtype, device='meta')}
    if strides == _dense(shape):
        bad['a strided row view'] = _view(shape, (strides[0] + 16,) + strides[1:], dtype)
    else:
        bad['contiguous'] = _view(shape, _dense(shape), dtype)
    if align > torch.empty(0, dtype=dtype).element_size():
        bad['alignment'] = _view(shape, strides, dtype, offset=1)
        assert bad['alignment'].data_ptr() % align
    return bad


@case_of
def test_a_wrong_out_is_a_value_error_before_the_library_is_reached(case, monkeypatch):
    n = case.n

    def rejected(names, out, why):
        calls = []
        with pytest.raises(ValueError):
            calls = _run(case, monkeypatch, n, names, out)[1]
        assert not calls, (case.name, why)

    good = {k: _view(*[case.spec(n)[k][i] for i in (0, 2, 1)]) for k in case.outputs}
    assert all(a is b for a, b in zip(_run(case, monkeypatch, n, case.outputs, dict(good))[0].values(), good.values()))
    for k in case.outputs:
        for why, t in _wrong(case, n, k).items():
            rejected(case.outputs, dict(good, **{k: t}), (k, why))
            rejected(case.outputs, {k: t}, (k, why))
        rejected(case.outputs, {k: 'a string'}, (k, 'no tensor'))
    if case.keyed:
        rejected(case.outputs, dict(good, nope=good[case.outputs[0]]), 'an unknown key')
        for names in case.subsets()[1:]:
            for k in case.outputs:
                if k not in names:
                    rejected(names, {k: good[k]}, ('a key the call does not write', names, k))


@case_of
def test_empty_tensors_of_any_stride_are_accepted(case, monkeypatch):
    spec = case.spec(0)
    # (strides of 72 in front of a unit one: recall's `record` is viewed as float32 and int16, which takes a dense last
    # dimension and whole elements between the rows)
    out = {k: _view(spec[k][0], (72,) * (len(spec[k][0]) - 1) + (1,), spec[k][1]) for k in case.outputs}
    assert all(tuple(t.stride()) != case.spec(0)[k][2] for k, t in out.items() if t.dim() > 1)
    res, calls = _run(case, monkeypatch, 0, case.outputs, dict(out), forbid=('empty', 'zeros', 'as_strided'))
    assert all(res[k] is out[k] for k in case.outputs)
    assert len(calls) == int(case.launches_empty)
    new, calls = _run(case, monkeypatch, 0, case.outputs)
    _as_documented(case, 0, new)
    assert len(calls) == int(case.launches_empty)
    if calls:
        assert [p or 0 for p in case.pointers(calls[0])] == [new[k].data_ptr() for k in case.outputs]


def test_check_outputs_orders_the_names_and_rejects_none_and_unknown_ones():
    for name in ('peek', 'peek_dict', 'worth', 'relabel', 'recall'):
        mod = importlib.import_module('gridworld_amd.' + name)
        assert mod.check_outputs(mod.OUTPUTS) == mod.OUTPUTS
        assert mod.check_outputs(list(reversed(mod.OUTPUTS))) == mod.OUTPUTS
        assert mod.check_outputs(mod.OUTPUTS[-1:] + mod.OUTPUTS[:1]) == mod.OUTPUTS[:1] + mod.OUTPUTS[-1:]
        for bad in ((), [], ('nope',), mod.OUTPUTS + ('nope',)):
            with pytest.raises(ValueError, match=name + ': outputs names'):
                mod.check_outputs(bad)
        one = mod.OUTPUTS[1]
        if name in ('peek', 'peek_dict'):          # a bare string is its letters
            with pytest.raises(ValueError, match=name + ': outputs names'):
                mod.check_outputs(one)
        else:
            assert mod.check_outputs(one) == (one,)


@pytest.mark.parametrize('name, word', [('relabel', 'relabel: grids'), ('recall', 'recall: starts')])
def test_grid_rows_takes_three_shapes_and_keeps_a_tensor_that_is_right_already(name, word):
    mod = importlib.import_module('gridworld_amd.' + name)
    lead = (2, 3)
    cells = torch.arange(2 * 3 * 1089).reshape(lead + (1089,)) % 7
    want = torch.zeros(lead + (ROW,), dtype=torch.int8)
    want[..., :1089] = cells.to(torch.int8)
    for x in (cells.reshape(lead + (9, 11, 11)), cells, cells.numpy(), want.to(torch.int32), want.clone()):
        got = mod.grid_rows(x, CPU, lead)
        assert got.dtype == torch.int8 and tuple(got.shape) == lead + (ROW,) and got.is_contiguous()
        assert torch.equal(got, want)
    assert mod.grid_rows(want, CPU, lead) is want
    part = want[0]
    assert mod.grid_rows(part, CPU, (3,)) is part
    for bad in (torch.zeros(lead + (1088,), dtype=torch.int8), torch.zeros((3, 2, 1089), dtype=torch.int8),
                torch.zeros(lead + (9, 11, 12), dtype=torch.int8)):
        with pytest.raises(ValueError, match=word):
            mod.grid_rows(bad, CPU, lead)


def test_the_other_row_readers_stay_reachable_under_their_names():
    from gridworld_amd import recall, vox
    t = torch.zeros((2, 2, 9, 11, 11), dtype=torch.int8)
    assert recall.goal_rows(t) == (t.data_ptr(), 1089, 4)
    wide = torch.as_strided(torch.zeros((2, ROW), dtype=torch.int8), (2, 9, 11, 11), GRID)
    assert vox.rows_of('grid', wide, 2) == (wide.data_ptr(), ROW)

"""What the query modules' launch() functions share on the host: the one path from `out` to the tensors a call writes and
the pointers its library entry takes, and the small argument checks.  torch is imported inside the functions, so a
module's build() works without it."""
CELLS, ROW = 1089, 1104      # the cells of a grid and the bytes of its row (include/igw.h)


def spec(shape, dtype, strides=None, align=1, rows=None, zero=False):
    """One entry of a query's output table: the `shape` and `dtype` a caller sees; its `strides`, or None for a
    contiguous tensor; the alignment in bytes the library asks of its address; `rows`, the shape of the allocation a
    strided output is a view of; and whether that allocation is zero-filled (its padding is visible)."""
    return shape, strides, dtype, align, rows or shape, zero


def outputs(query, order, names, specs, out, dev, alloc_stream=None):
    """(name -> tensor for `names`, the pointers in `order` with None for what is not in `names`) of one call of
    `query`: the tensors of `out` (a dict or None) as they are, after a check against `specs` (name -> spec()), and new
    ones, allocated on `alloc_stream`, for the rest.  With every output given no torch operation runs.  The strides of
    an empty tensor are not looked at."""
    import torch
    out = dict(out or {})
    unknown = [k for k in out if k not in names]
    if unknown:
        raise ValueError(f'out holds {unknown}, the call writes {list(names)}')
    for k, t in out.items():
        shape, strides, dtype, align, _, _ = specs[k]
        if (not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dtype or t.device != dev
                or (not t.is_contiguous() if strides is None else t.numel() > 0 and tuple(t.stride()) != strides)
                or t.data_ptr() % align):
            layout = 'contiguous' if strides is None else f'with strides {strides}'
            raise ValueError(f'out[{k!r}] must be a {dtype} tensor {shape}, {layout}, on {dev}, {align}-byte aligned '
                             f'(what {query}() returns)')
    missing = [k for k in names if k not in out]
    if missing:
        with torch.cuda.stream(alloc_stream):
            for k in missing:
                shape, strides, dtype, _, rows, zero = specs[k]
                t = (torch.zeros if zero else torch.empty)(rows, dtype=dtype, device=dev)
                out[k] = t if strides is None else torch.as_strided(t, shape, strides)
    return {k: out[k] for k in order if k in names}, [out[k].data_ptr() if k in names else None for k in order]


def ptr(x):
    return None if x is None else x.data_ptr()


def check_outputs(query, order, outputs, string=True):
    """The outputs named, in the library's `order`; ValueError for none or an unknown one.  string=False: a bare string
    is not one name but its letters (peek, peek_dict)."""
    names = (outputs,) if string and isinstance(outputs, str) else tuple(outputs)
    if not names or any(k not in order for k in names):
        some, got = ('one or more of', outputs) if string else ('some of', names)
        raise ValueError(f'{query}: outputs names {some} {order}{"" if string else ", at least one"}, got {got!r}')
    return tuple(k for k in order if k in names)


def _is(t, dtype, shape, dev):
    import torch
    return (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.device == dev
            and t.is_contiguous())


def grid_rows(what, x, dev, lead):
    """An integer tensor or array [*lead, 9, 11, 11], [*lead, 1089] or [*lead, 1104] -> a contiguous int8 device tensor
    [*lead, 1104] (the one given, if it is that already); `what` ('relabel: grids') opens the ValueError's message."""
    import numpy as np
    import torch
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    lead = tuple(lead)
    if tuple(t.shape) == lead + (9, 11, 11):
        t = t.reshape(lead + (CELLS,))
    if tuple(t.shape) == lead + (ROW,):
        return t.to(device=dev, dtype=torch.int8).contiguous()
    if tuple(t.shape) != lead + (CELLS,):
        raise ValueError(f'{what} must be {lead + (9, 11, 11)}, {lead + (CELLS,)} or {lead + (ROW,)}, got {tuple(t.shape)}')
    rows = torch.zeros(lead + (ROW,), dtype=torch.int8, device=dev)
    rows[..., :CELLS] = t.to(device=dev, dtype=torch.int8)
    return rows

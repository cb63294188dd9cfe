"""Model of the training-layout observation (include/igw_render.h: igw_render_obs; DESIGN.md section 8,
"Training-layout observations"), written from the contract and not from the kernel: plain torch ops that run wherever
the frames live.

    stack = obs_model.observe(frames, prev, restart, spec)

frames uint8 [N, H, W, 3] (what render_pov() draws), prev the stack the previous call returned (None: every env
restarts), restart a mask [N] (None: nobody restarts; any value != 0 counts) and spec a render.ObsSpec; returns
[N, K * planes, H, W] of spec.dtype.  The float path is two separate ops, mul then add, then .to(dtype): each rounds
once (no addcmul, no fused multiply-add)."""
import torch


def luminance(frames):
    """uint8 [...] Y of uint8 RGB [..., 3]: (19595 R + 38470 G + 7471 B + 32768) >> 16, the codec's Y."""
    r, g, b = (frames[..., k].to(torch.int64) for k in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).to(torch.uint8)


def planes(frames, spec):
    """uint8 [N, planes, H, W]: the luminance plane, or R, G, B channel-first."""
    if spec.gray:
        return luminance(frames).unsqueeze(1)
    return frames[..., :3].permute(0, 3, 1, 2).contiguous()


def convert(v, spec):
    """The stored value of uint8 `v` in spec.dtype."""
    if spec.dtype is torch.uint8:
        return v
    f = v.to(torch.float32)
    f = torch.mul(f, torch.tensor(spec.scale, dtype=torch.float32, device=v.device))
    f = torch.add(f, torch.tensor(spec.bias, dtype=torch.float32, device=v.device))
    return f.to(spec.dtype)


def observe(frames, prev, restart, spec, fill=False):
    new = convert(planes(frames, spec), spec)                       # [N, P, H, W]
    N, P, H, W = new.shape
    K = spec.stack
    filled = new.unsqueeze(1).expand(N, K, P, H, W)
    if prev is None or fill:
        return filled.reshape(N, K * P, H, W).contiguous()
    shifted = torch.cat([prev.reshape(N, K, P, H, W)[:, 1:], new.unsqueeze(1)], 1)
    if restart is None:
        return shifted.reshape(N, K * P, H, W).contiguous()
    r = torch.as_tensor(restart, device=new.device).reshape(N).ne(0)
    return torch.where(r.view(N, 1, 1, 1, 1), filled, shifted).reshape(N, K * P, H, W).contiguous()


def bits(t):
    """The raw bits of a tensor as an integer tensor (what torch.equal compares: -0.0 and NaN payloads included)."""
    return t if t.dtype is torch.uint8 else t.view({2: torch.int16, 4: torch.int32}[t.element_size()])

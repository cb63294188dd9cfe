"""What the render tests share (next to the model, tests/pov_model.py): the comparison of frames against the model
with the project's limits, the reference's atlas, and the cross-compiled library's code object and its gates."""
import ctypes
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import pov_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = '/opt/rocm/lib/llvm/bin'


def _ref_atlas():
    return np.load(os.path.join(HERE, 'golden', 'texture_atlas.npz'))['atlas']


def _models(poses, grids, W, H, atlas):
    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda k: M.render(poses[k], grids[k], atlas, W, H, 4), range(len(poses))))


class Tally:
    """Mismatches of frames against the model: none outside the boundary band, <= 0.1 % of the pixels inside it."""

    def __init__(self, what):
        self.what, self.clean_bad, self.band_bad, self.n, self.notes = what, 0, 0, 0, []

    def add(self, frame, res, channels, tag=''):
        r = dict(res, image=res['image'][..., :channels])
        c, b, n = M.compare(frame, r)
        if c:   # a finding: report the pixels with their margins
            bad = (np.asarray(frame) != r['image']).any(-1) & M.clean(r)
            for i, j in np.argwhere(bad)[:5]:
                self.notes.append(f'{tag} pixel ({i}, {j}): face {r["face"][i, j]}, t {r["t"][i, j]:.4f}, texel margin '
                                  f'{r["margin_texel"][i, j]:.3g}, world margin {r["margin_world"][i, j]:.3g}')
        self.clean_bad += c
        self.band_bad += b
        self.n += n

    def check(self):
        print(f'{self.what}: {self.n} pixels, {self.clean_bad} mismatches outside the band, {self.band_bad} inside '
              f'({100.0 * self.band_bad / max(self.n, 1):.4f} % of the pixels; the limit is 0.1 %)')
        for note in self.notes:
            print('  ' + note)
        assert self.clean_bad == 0, self.notes
        assert self.band_bad <= 1e-3 * self.n


def _kernel_notes_and_asm(tmp_path):
    """(notes, disassembly) of the gfx950 code object inside libigw_render.so."""
    from gridworld_amd import render as R
    lib = R.build()
    tools = [os.path.join(LLVM, t) for t in ('llvm-objcopy', 'clang-offload-bundler', 'llvm-readelf', 'llvm-objdump')]
    fat, co = str(tmp_path / 'fat.bin'), str(tmp_path / 'dev.co')
    subprocess.check_call([tools[0], '--dump-section', '.hip_fatbin=' + fat, lib])
    subprocess.check_call([tools[1], '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--input=' + fat,
                           '--output=' + co, '--unbundle'])
    notes = subprocess.check_output([tools[2], '--notes', co], text=True)
    asm = subprocess.check_output([tools[3], '-d', co], text=True)
    return notes, asm


def _forbidden(asm):
    return re.search(r'\bs_(buffer_)?(store|atomic)|\bs_scratch_|\bscratch_', asm)


def _kernel_gates(notes, asm, name):
    """The gates every kernel of the library passes; returns (the kernel's notes, val(key) of them, its body)."""
    blocks = notes.split('- .agpr_count:')[1:]
    kern = [b for b in blocks if name in b]
    assert len(kern) == 1
    val = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, kern[0]).group(1))  # noqa: E731
    print('%s: %d VGPRs, %d SGPRs, %d B of LDS' % (name, val('vgpr_count'), val('sgpr_count'),
                                                   val('group_segment_fixed_size')))
    assert val('private_segment_fixed_size') == 0
    assert val('vgpr_spill_count') == 0 and val('sgpr_spill_count') == 0
    assert val('vgpr_count') <= 128
    assert val('group_segment_fixed_size') <= 20 * 1024
    body = re.search(r'^[0-9a-f]+ <\S*%s\S*>:\n(.*?)(?:\n\n|\Z)' % name, asm, re.M | re.S).group(1)
    assert not _forbidden(body)
    return kern[0], val, body


def _buffers():
    buf = (ctypes.c_uint8 * (1 << 16))()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    return buf, p16

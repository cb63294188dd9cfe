"""Prints the source hash (the build id a fresh build would carry) of every library of the package, one per line.

    python tools/build_ids.py

No compile and no device: the hash is over the sources, the headers and the compiler flags (build.Library.source_hash),
so two commits that print the same listing build byte-compatible ids -- staleness and the profile stamps do not move.
"""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUERIES = ('query', 'goal', 'aim', 'peek', 'peek_dict', 'vox', 'worth', 'relabel', 'recall')


def build_ids():
    from gridworld_amd import build, codec, render
    ids = {'step': build.STEP.source_hash(), 'diag': build.DIAG.source_hash(), 'render': render.LIBRARY.source_hash(),
           'render_obs': render.OBS_LIBRARY.source_hash(), 'codec': codec.LIBRARY.source_hash()}
    for name in QUERIES:
        ids[name] = importlib.import_module('gridworld_amd.' + name).LIBRARY.source_hash()
    return ids


if __name__ == '__main__':
    for name, h in build_ids().items():
        print(f'{name:<11}{h}')

"""Builds gridworld_amd/libigw_hip.so (HIP kernels + C ABI) for gfx950 with hipcc.

    python -m gridworld_amd.build            # build if stale: the step library, then the render, codec, query, goal,
    python -m gridworld_amd.build --force    # aim, peek, peek_dict, vox, worth, relabel and recall libraries (each module's own build())

hipcc cross-compiles without a GPU.  -ffp-contract=off is REQUIRED: the reference computes
in IEEE binary64 with one rounding per operation; never add fast-math flags.
"""
import ctypes
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libigw_hip.so')
LIB_DIAG = os.path.join(HERE, 'libigw_hip_diag.so')  # -DIGW_DIAG: phase stamps + ablation switches (tools/ only)
SOURCES = ['igw_kernels.hip']
HEADERS = ['igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h',
           os.path.join('..', '..', 'include', 'igw.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
         '-fno-fast-math', '-Wall', '-Wno-unused-variable', '-Wno-bitwise-instead-of-logical',
         # the step kernel's leading scalar arguments (the pointers of its input burst) arrive preloaded in SGPRs
         '-mllvm', '-amdgpu-kernarg-preload-count=7',
         # the counters are added by ONE lane per wavefront already (a ballot + popcount): the compiler's own wave-level
         # reduction in front of every atomic only adds a dozen instructions
         '-mllvm', '-amdgpu-atomic-optimizer-strategy=None']


def hipcc():
    for c in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if c and os.path.exists(c):
            return c
    raise RuntimeError('hipcc not found')


class Library:
    """One hipcc-built shared library: where it goes, what it is made of, and how its build id is stamped into it.
    `sources` and `headers` are file names (relative ones are looked up under `root`); `marker` is the string that
    precedes the id inside the file and `define` the macro that carries marker + id into the source; `flags` are
    added to FLAGS on the command line and `suffix` to the id; `deps` are further files a build is older than when
    it is stale (the module that describes the library)."""

    def __init__(self, lib, sources, headers, marker, define, root='', flags=(), suffix='', deps=()):
        self.lib, self.sources, self.headers, self.marker, self.define = lib, sources, headers, marker.encode(), define
        self.root, self.flags, self.suffix, self.deps = root, tuple(flags), suffix, [os.path.abspath(d) for d in deps]

    def path(self, name):
        return os.path.join(self.root, name)

    def source_hash(self):
        """Identity of a build: sha256 over the sources and headers (sorted by name; base name, NUL, contents) and the
        compiler FLAGS, 16 hex digits, plus the suffix."""
        import hashlib
        h = hashlib.sha256()
        for f in sorted(self.sources + self.headers):
            h.update(os.path.basename(f).encode() + b'\0')
            with open(self.path(f), 'rb') as fh:
                h.update(fh.read())
        h.update(' '.join(FLAGS).encode())
        return h.hexdigest()[:16] + self.suffix

    def built_id(self, lib=None):
        """The build id of an existing library file, read without loading it (the id string follows the marker)."""
        try:
            with open(lib or self.lib, 'rb') as f:
                data = f.read()
            i = data.find(self.marker)
            if i < 0:
                return None
            return data[i + len(self.marker):data.index(b'\0', i)].decode()
        except (OSError, ValueError):
            return None

    def is_stale(self, lib=None):
        """Missing, older than a source (mtime), or built from other sources than the ones on disk (build id)."""
        lib = lib or self.lib
        if not os.path.exists(lib):
            return True
        t = os.path.getmtime(lib)
        deps = [self.path(f) for f in self.sources + self.headers] + self.deps
        return any(os.path.getmtime(d) > t for d in deps) or self.built_id(lib) != self.source_hash()

    def build(self, force=False, extra_flags=(), verbose=False):
        """Compiles under an exclusive file lock and installs the result with an atomic rename, so several
        ranks starting at once (torchrun) never see or write a half-built library."""
        lib = self.lib
        if not force and not self.is_stale():
            return lib
        import fcntl
        with open(lib + '.lock', 'w') as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if not force and not self.is_stale():  # another process built it while we waited
                    return lib
                tmp = f'{lib}.tmp.{os.getpid()}'
                stamp = '-D%s="%s%s"' % (self.define, self.marker.decode(), self.source_hash())
                cmd = ([hipcc()] + FLAGS + list(extra_flags) + list(self.flags) + [stamp, '-o', tmp]
                       + [self.path(s) for s in self.sources])
                if verbose:
                    print(' '.join(cmd))
                subprocess.run(cmd, check=True)
                os.replace(tmp, lib)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
        return lib

    def build_for_load(self, error):
        """The rule of a binding that builds before it loads: a compile error raises `error` (never a fall back to a
        stale binary); without a compiler an existing library is still usable, a missing one is fatal."""
        name = os.path.basename(self.lib)
        try:
            self.build()
        except subprocess.CalledProcessError as e:
            raise error(f'hipcc failed to build {name}: {e}') from e
        except Exception as e:
            if not os.path.exists(self.lib):
                raise error(f'{name} is missing and could not be built: {e}') from e


class Binding:
    """The ctypes side of a Library: load() types every symbol of `signatures` (name -> (result, arguments)), check()
    turns a nonzero return code into `error` with the text of the `last_error` symbol, build_id() calls the
    `build_id` symbol.  `module` is what the "not found" message says to run; `what` is check()'s default entry."""

    def __init__(self, library, signatures, error, last_error, build_id, module, what):
        self.library, self.signatures, self.error, self.module, self.what = library, signatures, error, module, what
        self._last_error, self._build_id = last_error, build_id
        self.lib = None

    def load(self, build_if_missing=True):
        """Loads the library, building it first if it is missing or stale; a failed compile raises."""
        if self.lib is not None:
            return self.lib
        if build_if_missing:
            self.library.build_for_load(self.error)
        if not os.path.exists(self.library.lib):
            raise self.error(f'{os.path.basename(self.library.lib)} not found; run `python -m {self.module}`')
        lib = ctypes.CDLL(self.library.lib)
        for name, (res, args) in self.signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        self.lib = lib
        return lib

    def build_id(self):
        return getattr(self.load(), self._build_id)().decode()

    def check(self, code, what=None):
        if code != 0:
            msg = getattr(self.load(), self._last_error)()
            raise self.error(f'{what or self.what} failed ({code}): {msg.decode() if msg else ""}')


# What a library that reads the step path's state includes: the device headers and the step ABI (absolute paths, as a
# query module's own files are).
DEVICE_HEADERS = [os.path.join(CSRC, f) for f in ('igw_device.h', 'igw_trig.h', 'igw_trig_lut.h', 'igw_trig_tables.h')] + \
                 [os.path.join(HERE, '..', 'include', 'igw.h')]


def query(name, module_file, signatures, error, what, headers=(), include=(), device=True):
    """(Library, Binding) of the query library `name`: libigw_<name>.so from csrc/<name>/igw_<name>.hip, the headers
    `headers` under csrc and include/igw_<name>.h (after `include`, further ones of include/) -- behind DEVICE_HEADERS
    when the kernels read the step path's state.  `signatures` are the entry points; the three symbols every library has
    (igw_<name>_version / _build_id / _last_error) are put in front of them.  `error` is what the binding raises, `what`
    the entry check() names by default, `module_file` the describing module: the library is stale when that file or this
    one is newer."""
    sym = 'igw_' + name
    lib = Library(os.path.join(HERE, f'lib{sym}.so'), [os.path.join(CSRC, name, sym + '.hip')],
                  (DEVICE_HEADERS if device else []) + [os.path.join(CSRC, f) for f in headers] +
                  [os.path.join(HERE, '..', 'include', f) for f in (*include, sym + '.h')],
                  f'igw-{name.replace("_", "-")}-build-id:', f'IGW_{name.upper()}_BUILD_ID', deps=[module_file, __file__])
    signatures = {sym + '_version': (ctypes.c_int, []), sym + '_build_id': (ctypes.c_char_p, []),
                  sym + '_last_error': (ctypes.c_char_p, []), **signatures}
    return lib, Binding(lib, signatures, error, sym + '_last_error', sym + '_build_id', 'gridworld_amd.' + name, what)


# The step library and its diagnostic variant (libigw_hip_diag.so, -DIGW_DIAG, next to the production library).  The
# id is compiled into the library (-DIGW_BUILD_ID, exported as igw_build_id()) and stamped on every profile summary
# under profiles/ (tools/summarize_profile.py), so a bench line can tell whether the PMC bytes it quotes were measured
# on the kernels it timed.
STEP = Library(LIB, SOURCES, HEADERS, 'igw-build-id:', 'IGW_BUILD_ID', root=CSRC, deps=[__file__])
DIAG = Library(LIB_DIAG, SOURCES, HEADERS, 'igw-build-id:', 'IGW_BUILD_ID', root=CSRC, flags=['-DIGW_DIAG'],
               suffix='-diag', deps=[__file__])


def source_hash(diag=False):
    return (DIAG if diag else STEP).source_hash()


def built_id(lib=LIB):
    return STEP.built_id(lib)


def is_stale(lib=LIB, diag=False):
    return (DIAG if diag else STEP).is_stale(lib)


def build(force=False, extra_flags=(), verbose=False, diag=False):
    return (DIAG if diag else STEP).build(force, extra_flags, verbose)


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True, diag='--diag' in sys.argv))
    if '--diag' not in sys.argv:   # ... and the libraries beside the step library, each by its own module's build()
        from . import aim, codec, goal, peek, peek_dict, query, recall, relabel, render, vox, worth
        for module in (render, codec, query, goal, aim, peek, peek_dict, vox, worth, relabel, recall):
            print(module.build(force='--force' in sys.argv))

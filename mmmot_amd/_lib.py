"""Loader and builder of ``libmmmot_hip.so`` (the C-ABI of include/mmmot_hip.h).

The library is built in-tree with ``hipcc --offload-arch=gfx950`` (no torch
headers, no CMake) and loaded with ctypes.  There is NO fallback: if the shared
object is missing or fails to load, every op raises - the product path never
computes on the CPU.
"""
import collections
import ctypes
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.environ.get('MMMOT_LIB_PATH', os.path.join(_HERE, 'libmmmot_hip.so'))  # override: tools' timing-experiment builds
SOURCES = [
    'conv3x3.hip', 'hl16_format.hip', 'conv3x3_hl16_patch.hip', 'gemm_rows.hip', 'gemm_wide.hip', 'gemm_ares.hip',
    'gemm_wres.hip', 'gemm_wreg.hip', 'pn_mlp64.hip', 'gram.hip', 'points_gather.hip', 'crop_resize.hip',
    'crop_augment.hip', 'small_kernels.hip', 'backward.hip', 'train.hip', 'train_vgg.hip', 'gemm_tn_f16.hip',
    'assign.hip', 'assign_chain.hip', 'assign_sequence.hip', 'track_ids.hip', 'clear_mot.hip', 'hota.hip',
    'mot3d.hip', 'align_points.hip', 'fill_tracks.hip', 'labels.hip', 'adam_step.hip', 'dropout.hip',
    'gate_links.hip', 'smooth_tracks.hip', 'stitch_tracks.hip',
]
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
HIPFLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC']

HEADER = os.path.join(_HERE, '..', 'include', 'mmmot_hip.h')

_lock = threading.Lock()
_lib = None

# ---- the binding is derived from the header: one declaration per entry point, in plain C ----
c_i = ctypes.c_int
_SCALARS = {'int': c_i, 'long': ctypes.c_long, 'long long': ctypes.c_longlong, 'unsigned': ctypes.c_uint,
            'unsigned int': ctypes.c_uint, 'unsigned long long': ctypes.c_ulonglong, 'float': ctypes.c_float,
            'double': ctypes.c_double}
_POINTEES = set(_SCALARS) | {'void', 'char', 'unsigned char'}
# structs of the header that travel by pointer and are filled from Python -> name of their ctypes mirror
MIRRORS = {'mmmot_gemm_args': 'GemmArgs', 'mmmot_gemm_ares_args': 'GemmAresArgs', 'mmmot_gemm_tn_args': 'GemmTnArgs'}

# one parameter (or struct field): ctype is what ctypes binds; pointee the C type a pointer points to (None: a scalar).
# Device and host pointers alike travel as integers (c_void_p), except a mirrored struct's and `char*`
Param = collections.namedtuple('Param', 'name ctype pointee')


def _declarator(decl, structs, where):
    """'const float* X' -> Param('X', c_void_p, 'float'); anything the header's plain C does not use raises"""
    head, star, name = re.sub(r'\bconst\b', ' ', decl).strip().rpartition('*')
    if not star:
        head, _, name = name.rpartition(' ')
    base, name = ' '.join(head.split()), name.strip()
    if name.isidentifier():
        if not star and base in _SCALARS:
            return Param(name, _SCALARS[base], None)
        if star and isinstance(structs.get(base), type):
            return Param(name, ctypes.POINTER(structs[base]), base)
        if star and (base in _POINTEES or base in structs):
            return Param(name, ctypes.c_char_p if base == 'char' else ctypes.c_void_p, base)
    raise ValueError('%s: cannot bind "%s" (include/mmmot_hip.h stays within int / long / float / double scalars and '
                     'single pointers, one declarator per `;` in structs)' % (where, decl.strip()))


def parse_header(text):
    """(structs, params, debug_params) of the header's text: the ctypes mirrors of the MIRRORS structs by C name (every
    other struct: None, an opaque pointee) and, per `int mmmot_x(...);` prototype, its list of Param - the ones inside
    `#ifdef MMMOT_DEBUG` apart."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    structs = {}
    for cname, body in re.findall(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;', text, flags=re.S):
        structs[cname] = None
        if cname in MIRRORS:
            fields = [_declarator(f, structs, 'struct ' + cname) for f in body.split(';') if f.strip()]
            structs[cname] = type(MIRRORS[cname], (ctypes.Structure,), {
                '__doc__': 'Mirror of ``%s`` (include/mmmot_hip.h).' % cname,
                '_fields_': [(f.name, f.ctype) for f in fields]})
    found = {}
    for debug, part in enumerate(re.split(r'#ifdef MMMOT_DEBUG(.*?)#endif', text, flags=re.S)):
        for name, args in re.findall(r'\bint\s+(mmmot_\w+)\s*\(([^)]*)\)\s*;', part):
            args = [] if args.strip() == 'void' else args.split(',')
            found[name] = (debug % 2, [_declarator(a, structs, name) for a in args])
    return (structs, {n: p for n, (d, p) in found.items() if not d}, {n: p for n, (d, p) in found.items() if d})


with open(HEADER) as _f:
    _STRUCTS, PARAMS, DEBUG_PARAMS = parse_header(_f.read())
GemmArgs, GemmAresArgs, GemmTnArgs = (_STRUCTS[c] for c in MIRRORS)
# name -> argtypes; every entry point declared in include/mmmot_hip.h
SIGNATURES = {name: [p.ctype for p in params] for name, params in PARAMS.items()}
# entry points that exist only in -DMMMOT_DEBUG builds (timing experiments of tools/; never the product library)
DEBUG_SIGNATURES = {name: [p.ctype for p in params] for name, params in DEBUG_PARAMS.items()}
# the entries that launch: their last parameter is `void* stream`
TAKES_STREAM = frozenset(n for n, p in PARAMS.items() if p and p[-1] == ('stream', ctypes.c_void_p, 'void'))
DEBUG_LIB_PATH = os.path.join(_HERE, 'libmmmot_hip_debug.so')


def build(force=False, verbose=False, debug=False):
    """Compile every HIP source for gfx950 and link libmmmot_hip.so in-tree.  ``debug=True`` builds the
    -DMMMOT_DEBUG variant (timing experiments of the patch kernel) as libmmmot_hip_debug.so; load it by setting
    MMMOT_LIB_PATH before importing mmmot_amd (tools/ do)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    # headers and the textual parts of the trunk kernel (csrc/patch_*.inc): any of them newer than the library rebuilds it
    deps = srcs + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(('.h', '.inc'))] + [HEADER]
    lib_path = DEBUG_LIB_PATH if debug else LIB_PATH
    if not force and os.path.exists(lib_path):
        if all(os.path.getmtime(lib_path) >= os.path.getmtime(d) for d in deps):
            return lib_path
    objs = []
    procs = []
    for s in srcs:
        o = s[:-4] + ('.dbg.o' if debug else '.o')
        objs.append(o)
        cmd = [HIPCC] + HIPFLAGS + (['-DMMMOT_DEBUG'] if debug else []) + ['-c', s, '-o', o]
        if verbose:
            print(' '.join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError('hipcc failed: %s\n%s' % (' '.join(cmd), out.decode()))
    cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib_path] + objs
    if verbose:
        print(' '.join(cmd))
    subprocess.check_call(cmd)
    return lib_path


def load():
    """Return the ctypes handle; raises (never falls back) when unavailable."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    'libmmmot_hip.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
                    'g.build()"`. There is no CPU fallback for the HIP path.' % LIB_PATH)
            lib = ctypes.CDLL(LIB_PATH)
            # MMMOT_LIB_ALLOW_MISSING=1 (tools/ab_forward.py only: an OLDER build of the library beside the current one)
            # tolerates entry points the other build does not have yet; the product never sets it
            lenient = os.environ.get('MMMOT_LIB_ALLOW_MISSING', '0') == '1'
            for name, argtypes in SIGNATURES.items():
                fn = getattr(lib, name, None) if lenient else getattr(lib, name)  # AttributeError if the symbol is missing
                if fn is None:
                    continue
                fn.argtypes = argtypes
                fn.restype = c_i
            for name, argtypes in DEBUG_SIGNATURES.items():  # present in -DMMMOT_DEBUG builds only
                fn = getattr(lib, name, None)
                if fn is not None:
                    fn.argtypes = argtypes
                    fn.restype = c_i
            _lib = lib
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError('%s failed with status %d%s' % (
            what, status, ' (MMMOT_EINVAL: contract violation)' if status == -1 else ' (hipError_t)'))

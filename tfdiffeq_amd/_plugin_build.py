"""Compile and load right-hand-side plugins (csrc/mi_ode_plugin.h and the other kinds' headers: KINDS): hipcc, gfx950, cached by source hash."""
import collections
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

from . import _native as N

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-shared',
         '-I', N.CSRC, '-I', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include')]
_loaded = {}
_tables = {}         # (kind, source, dtype) -> (library, table address): load()

# The kinds of plugin: one row each.  `base` is the kind whose translation unit a derived kind is written from (derive() swaps the header
# and the macro; None: the unit is generated as it is - rhs.CustomRowLocal / rhs.CustomCoop / lower), `not_base` the ValueError text when
# derive() is handed something else (None: lenient - the text is returned with nothing replaced), `label` names the kind in load()'s error.
Kind = collections.namedtuple('Kind', 'name header macro getter base not_base label')
KINDS = {k.name: k for k in (
    Kind('row-local', 'mi_ode_plugin.h', 'MI_ODE_DEFINE_ROWLOCAL_PLUGIN', 'mi_ode_plugin_get', None, None, 'plugin'),
    Kind('coop', 'mi_ode_plugin.h', 'MI_ODE_DEFINE_COOP_PLUGIN', 'mi_ode_plugin_get', None, None, 'plugin'),
    Kind('hyper', 'mi_ode_hyper_plugin.h', 'MI_ODE_DEFINE_HYPER_PLUGIN', 'mi_ode_hyper_plugin_get', 'row-local', None, 'hyper plugin'),
    Kind('rows', 'mi_ode_rows_plugin.h', 'MI_ODE_DEFINE_ROWS_PLUGIN', 'mi_ode_rows_plugin_get', 'row-local',
         'not a row-local plugin translation unit: the per-trajectory kernel takes one trajectory per thread', 'rows plugin'),
    Kind('rows-t', 'mi_ode_rows_t_plugin.h', 'MI_ODE_DEFINE_ROWS_T_PLUGIN', 'mi_ode_rows_t_plugin_get', 'row-local',
         'not a row-local plugin translation unit: the per-trajectory kernel takes one trajectory per thread', 'rows-t plugin'),
    Kind('fixed-rows-t', 'mi_ode_fixed_rows_t_plugin.h', 'MI_ODE_DEFINE_FIXED_ROWS_T_PLUGIN', 'mi_ode_fixed_rows_t_plugin_get', 'row-local',
         'not a row-local plugin translation unit: the fixed-grid kernel with per-row times takes one trajectory per thread', 'fixed-rows-t plugin'),
    Kind('discrete', 'mi_ode_discrete_plugin.h', 'MI_ODE_DEFINE_DISCRETE_PLUGIN', 'mi_ode_discrete_plugin_get', None, None, 'discrete plugin'),
    Kind('discrete-t', 'mi_ode_discrete_t_plugin.h', 'MI_ODE_DEFINE_DISCRETE_T_PLUGIN', 'mi_ode_discrete_t_plugin_get', 'discrete',
         'not a discrete plugin translation unit: the reverse sweep takes f with its generated vjp', 'discrete-t plugin'),
    Kind('hyper-grad', 'mi_ode_hyper_grad_plugin.h', 'MI_ODE_DEFINE_HYPER_GRAD_PLUGIN', 'mi_ode_hyper_grad_plugin_get', 'discrete',
         'not a discrete plugin translation unit: the hypersolver gradient takes f with its generated vjp', 'hyper-grad plugin'),
    Kind('rows-adjoint', 'mi_ode_rows_adjoint_plugin.h', 'MI_ODE_DEFINE_ROWS_ADJOINT_PLUGIN', 'mi_ode_rows_adjoint_plugin_get', None, None,
         'rows-adjoint plugin'),
    Kind('rows-adjoint-t', 'mi_ode_rows_adjoint_t_plugin.h', 'MI_ODE_DEFINE_ROWS_ADJOINT_T_PLUGIN', 'mi_ode_rows_adjoint_t_plugin_get', 'rows-adjoint',
         'not a rows-adjoint plugin translation unit: the per-row adjoint kernel takes f with its generated vjp', 'rows-adjoint-t plugin'),
)}


def _owned_private(path):
    """True if `path` belongs to this user and nobody else may write to it (what gets dlopen'ed must not be
    plantable by another account of the host)."""
    try:
        st = os.stat(path)
    except OSError:
        return False
    return st.st_uid == os.getuid() and (st.st_mode & 0o022) == 0


def plugin_dir():
    d = os.environ.get('TFDIFFEQ_AMD_PLUGIN_DIR')
    if not d:
        d = os.path.join(os.path.dirname(os.path.abspath(__file__)), '_plugins')      # in-tree: travels with the checkout
    try:
        os.makedirs(d, mode=0o755, exist_ok=True)
        if os.access(d, os.W_OK) and _owned_private(d):
            return d
    except OSError:
        pass
    # package directory not writable (site-packages install): a per-user cache, never a world-shared /tmp path
    base = os.environ.get('XDG_CACHE_HOME') or os.path.join(os.path.expanduser('~'), '.cache')
    d = os.path.join(base, 'tfdiffeq_amd', 'plugins')
    try:
        os.makedirs(d, mode=0o700, exist_ok=True)
    except OSError:
        d = tempfile.mkdtemp(prefix='tfdiffeq_amd_plugins_')                            # 0700, unpredictable name
    if not _owned_private(d):
        raise N.NativeError('refusing to use the plugin cache %s: it is not owned by this user or is writable by others' % d)
    return d


def _plugin_headers(roots=('mi_ode_plugin.h',)):
    """The headers a plugin translation unit actually sees: the #include closure of its own includes (mi_ode_plugin.h, or
    mi_ode_hyper_plugin.h for a hyper plugin) inside csrc/ and include/ (a change to the MLP / adjoint / linear-adjoint kernels does not
    invalidate the cache of compiled right-hand sides)."""
    import re
    inc = os.path.join(os.path.dirname(N.CSRC.rstrip(os.sep).rsplit(os.sep, 1)[0]), 'include')
    seen, todo = [], list(roots)
    while todo:
        name = todo.pop()
        for d in (N.CSRC, inc):
            path = os.path.join(d, os.path.basename(name))
            if os.path.exists(path) and path not in seen:
                seen.append(path)
                with open(path, 'r') as fh:
                    todo.extend(re.findall(r'^\s*#\s*include\s*"([^"]+)"', fh.read(), flags=re.M))
                break
    return sorted(seen)


def _source_roots(source):
    import re
    return tuple(re.findall(r'^\s*#\s*include\s*"([^"]+)"', source, flags=re.M)) or ('mi_ode_plugin.h',)


def _headers_digest(roots=('mi_ode_plugin.h',)):
    h = hashlib.sha256()
    for path in _plugin_headers(roots):
        with open(path, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(source, verbose=False):
    """Path of the compiled plugin for `source` (compiles on a cache miss; the key covers the kernel headers too)."""
    # (the include directories are NOT part of the key - their content is, through _headers_digest: a checkout that was moved, or copied to
    # another machine with its in-tree plugin cache, keeps hitting it)
    key = hashlib.sha256((source + _headers_digest(_source_roots(source)) + ' '.join(f for f in FLAGS if not os.path.isabs(f))).encode()).hexdigest()[:24]
    out = os.path.join(plugin_dir(), 'rhs_%s.so' % key)
    if os.path.exists(out):
        if not _owned_private(out):
            raise N.NativeError('refusing to load %s: not owned by this user or writable by others' % out)
        return out
    src = out[:-3] + '.hip'
    with open(src, 'w') as fh:
        fh.write(source)
    tmp = out + '.tmp%d' % os.getpid()
    limit = float(os.environ.get('TFDIFFEQ_AMD_PLUGIN_TIMEOUT_S', '600'))
    try:
        res = subprocess.run([HIPCC] + FLAGS + [src, '-o', tmp], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        for leftover in (tmp,):
            try:
                os.remove(leftover)
            except OSError:
                pass
        raise N.NativeError('compiling the RHS plugin failed: hipcc did not finish within %.0f s (TFDIFFEQ_AMD_PLUGIN_TIMEOUT_S); source: %s' % (limit, src))
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-6000:])
    if res.returncode != 0:
        raise N.NativeError('compiling the RHS plugin failed (hipcc output above); source: %s' % src)
    os.replace(tmp, out)
    return out


def build_and_load(source):
    path = build(source)
    lib = _loaded.get(path)
    if lib is None:
        import torch  # noqa: F401  (same reason as _native.load: bind to torch's HIP runtime)
        lib = C.CDLL(path)
        for name in getter_names():
            if hasattr(lib, name):
                getattr(lib, name).restype = C.c_void_p
                getattr(lib, name).argtypes = [C.c_int]
        _loaded[path] = lib
    return lib


def getter_names():
    """The getter symbols build_and_load declares on a library: the registry's, each once."""
    return tuple(dict.fromkeys(k.getter for k in KINDS.values()))


def derive(kind, source):
    """The translation unit of `kind` written from one of the kind it derives from: the same functor behind another header and macro."""
    k = KINDS[kind]
    base = KINDS[k.base]
    if k.not_base is not None and base.macro + '(' not in source:
        raise ValueError(k.not_base)
    src = source.replace('#include "%s"' % base.header, '#include "%s"' % k.header)
    return src.replace(base.macro + '(', k.macro + '(')


def load(kind, source, dtype):
    """(library, address of the table of `kind`) of a plugin translation unit; compiled once, cached by source and header hash."""
    key = (kind, source, dtype)
    hit = _tables.get(key)
    if hit is None:
        lib = build_and_load(source)
        table = getattr(lib, KINDS[kind].getter)(N.dtype_code(dtype))
        if not table:
            raise N.NativeError('%s exports no table for %s' % (KINDS[kind].label, dtype))
        hit = _tables[key] = (lib, int(table))
    return hit

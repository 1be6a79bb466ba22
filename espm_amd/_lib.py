"""ctypes binding of libespm_mu.so (include/espm_mu.h).

The HIP library is the product: there is NO CPU fallback.  A missing or stale library raises
at import of this module (``python -c "import __graft_entry__ as g; g.build()"`` rebuilds it).
"""
from __future__ import annotations

import ctypes as C
import os

# torch bundles its own HIP runtime (libamdhip64); it must be loaded FIRST so that libespm_mu.so binds
# to the same runtime instance as the tensors and streams it is handed (two runtimes in one process do
# not share devices: "no ROCm-capable device is detected").
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ESPM_MU_LIB", os.path.join(_HERE, "lib", "libespm_mu.so"))

from . import _abi

# ---- constants, enums, the state layout and every prototype come from include/espm_mu.h itself (espm_amd/_abi.py parses it):
# ---- no hand-kept copy of any of them ----
_HEADER_TEXT = _abi.header_text()
_D = _abi.parse_defines(_HEADER_TEXT)
_E = _abi.parse_enums(_HEADER_TEXT)
OK, EINVAL, ENOSOLUTION, EHIP, EUNSUPPORTED = (_E["ESPM_" + n] for n in ("OK", "EINVAL", "ENOSOLUTION", "EHIP", "EUNSUPPORTED"))   # enum espm_status
X_F32, X_BF16, X_U8, X_ELL = (_E["ESPM_X_" + n] for n in ("F32", "BF16", "U8", "ELL"))
F64_X_U8, F64_X_BF16, F64_X_F32, F64_X_F64 = (_D["ESPM_F64_X_" + n] for n in ("U8", "BF16", "F32", "F64"))
F64_MAX_K, F64_MAXIT = _D["ESPM_F64_MAX_K"], _D["ESPM_F64_MAXIT"]
F64S_MAX_COUNT, F64S_MAX_N, F64S_WBLOCK = _D["ESPM_F64S_MAX_COUNT"], _D["ESPM_F64S_MAX_N"], _D["ESPM_F64S_WBLOCK"]
DIAG_X_U8, DIAG_X_U16, DIAG_X_F32, DIAG_X_F64 = (_D["ESPM_DIAG_X_" + n] for n in ("U8", "U16", "F32", "F64"))
DIAG_MAX_K, DIAG_BLOCK, DIAG_CHUNK = _D["ESPM_DIAG_MAX_K"], _D["ESPM_DIAG_BLOCK"], _D["ESPM_DIAG_CHUNK"]
CDIAG_BLOCK, CDIAG_PCHUNK = _D["ESPM_CDIAG_BLOCK"], _D["ESPM_CDIAG_PCHUNK"]
BIN_BLOCK, BIN_PARTS = _D["ESPM_BIN_BLOCK"], _D["ESPM_BIN_PARTS"]
SPLIT_BLOCK, SPLIT_HEAVY, SPLIT_MAX_K = _D["ESPM_SPLIT_BLOCK"], _D["ESPM_SPLIT_HEAVY"], _D["ESPM_SPLIT_MAX_K"]
SAMPLE_BLOCK, SAMPLE_HEAVY, SAMPLE_MAX_RATE, SAMPLE_MAX_K = (_D["ESPM_SAMPLE_" + n] for n in ("BLOCK", "HEAVY", "MAX_RATE", "MAX_K"))
ATTRIB_BLOCK, ATTRIB_PCHUNK, ATTRIB_WALK, ATTRIB_HEAVY, ATTRIB_MAX_K = (_D["ESPM_ATTRIB_" + n] for n in ("BLOCK", "PCHUNK", "WALK", "HEAVY", "MAX_K"))
MARG_MAX_G, MARG_MAX_K, MARG_BLOCK, MARG_PCHUNK = (_D["ESPM_MARG_" + n] for n in ("MAX_G", "MAX_K", "BLOCK", "PCHUNK"))
MARG_PIXELS, MARG_CHANNELS = _E["ESPM_MARG_PIXELS"], _E["ESPM_MARG_CHANNELS"]
RESID_MAX_G, RESID_MAX_K, RESID_BLOCK, RESID_PCHUNK = (_D["ESPM_RESID_" + n] for n in ("MAX_G", "MAX_K", "BLOCK", "PCHUNK"))
RESID_PIXELS, RESID_CHANNELS = _E["ESPM_RESID_PIXELS"], _E["ESPM_RESID_CHANNELS"]
PML_MAX_K = _D["ESPM_PML_MAX_K"]
PMLN_STATE_EXTRA = _D["ESPM_PMLN_STATE_EXTRA"]   # espm_pixel_ml_newton's state: (k + PMLN_STATE_EXTRA, p) doubles
CML_STATE_EXTRA = _D["ESPM_CML_STATE_EXTRA"]     # espm_channel_ml_step's state: (n_models, 2 k + CML_STATE_EXTRA, n) doubles
PML_NOT_DONE, PML_UNMODELLED, PML_NONFINITE, PML_COUNTERS = (_E["ESPM_PML_" + n] for n in ("NOT_DONE", "UNMODELLED", "NONFINITE", "COUNTERS"))
SRC_F32, SRC_F64 =_E["ESPM_SRC_F32"], _E["ESPM_SRC_F64"]
LAYOUT_CM, LAYOUT_PM = _E["ESPM_LAYOUT_CM"], _E["ESPM_LAYOUT_PM"]
ABI_VERSION = _D["ESPM_MU_ABI_VERSION"]
XCHG_HANDLE_BYTES = _D["ESPM_XCHG_HANDLE_BYTES"]
ELL_TILE, ELL_PB, ELL_PBITS, ELL_LDS_MAX = _D["ESPM_ELL_TILE"], _D["ESPM_ELL_PB"], _D["ESPM_ELL_PBITS"], _D["ESPM_ELL_LDS_MAX"]
ELL_STREAM_BYTES = _D["ESPM_ELL_STREAM_BYTES"]
ELL_KEEP_BYTES = _D["ESPM_ELL_KEEP_BYTES"]
ELL_BUCKETS = _D["ESPM_ELL_BUCKETS"]
ELL_HEAVY_MIN, ELL_HEAVY_MAX = _D["ESPM_ELL_HEAVY_MIN"], _D["ESPM_ELL_HEAVY_MAX"]
ELL_UNIT_ROWS, ELL_UNIT_MAX_N, ELL_PAIR_MAX_K = _D["ESPM_ELL_UNIT_ROWS"], _D["ESPM_ELL_UNIT_MAX_N"], _D["ESPM_ELL_PAIR_MAX_K"]
KP, PPAD, NPAD = _D["ESPM_KP"], _D["ESPM_PPAD"], _D["ESPM_NPAD"]         # (the default build; `variant(k)` below for the wide one)
MAX_K = KP
HP_STRIDE, HS_STRIDE, HI_STRIDE = _D["ESPM_HP_STRIDE"], _D["ESPM_HS_STRIDE"], _D["ESPM_HI_STRIDE"]
HS_ROWSUM, HS_MAX = _D["ESPM_HS_ROWSUM"], _D["ESPM_HS_MAX"]
WIDE_MAX_K = 16      # libespm_mu_wide.so: 9..16 components (and the sparse count store's limit)
WIDEST_MAX_K = 32    # libespm_mu_wide32.so: 17..32 components, dense stores only
TAIL_DEFER, TAIL_RIDE = _D["ESPM_TAIL_DEFER"], _D["ESPM_TAIL_RIDE"]
HI_KLX, HI_REG, HI_LAP, HI_SUMY, HI_BAD, HI_REL_W, HI_REL_H = (_D["ESPM_HI_" + n] for n in ("KLX", "REG", "LAP", "SUMY", "BAD", "REL_W", "REL_H"))
# espm_mu_w_update_form: the forms of the W update by name, in the header's order
W_FORMS = {_D["ESPM_W_FORM_" + n]: n.lower() for n in ("LOCAL", "SIMPLEX_SPLIT", "DICT_COLUMNS", "DICT_TWO_LAUNCH", "ONE_WG_REGISTERS", "ONE_WG_GENERAL")}
W_FORMS_BY_NAME = {name: value for value, name in W_FORMS.items()}


def w_form_detail(detail):
    """espm_mu_w_update_form's `detail` unpacked (include/espm_mu.h: ESPM_W_DETAIL_*); {} for 0 - every form but the register-resident one."""
    if not detail:
        return {}
    return dict(threads=detail & 0xfff, rows=(detail >> 12) & 0xf, channels=(detail >> 16) & 0xf, gta_all_threads=bool((detail >> 20) & 1))


class MUState(C.Structure):
    """struct espm_mu_state: fields, order and types parsed from include/espm_mu.h.  A fresh instance carries
    struct_size / abi_version, which every entry point checks (ESPM_EINVAL on a mismatch)."""
    _fields_ = _abi.parse_struct(_HEADER_TEXT)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.struct_size = C.sizeof(type(self))
        self.abi_version = ABI_VERSION


# every function include/espm_mu.h declares: name -> (restype, argtypes), read from its declaration once per process
_SP = C.POINTER(MUState)
SYMBOLS = _abi.parse_prototypes(_HEADER_TEXT, _SP)


class EspmError(RuntimeError):
    """HIP runtime failure or unsupported configuration reported by libespm_mu."""


class LostPeerError(EspmError):
    """A sharded fit's one-shot record exchange gave up waiting for a peer: the iterates since then are not valid
    (MUEngine.history raises it on every rank at the same read-back; the estimator restarts on the collective transport)."""


def _load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP library is required (no CPU fallback). Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` at the repository root.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.restype, fn.argtypes = res, args
    # the library's view of the state against the header's: size, version, and every field's name, offset and size
    theirs, ours = lib.espm_mu_state_layout().decode(), _abi.layout_string(MUState)
    if lib.espm_mu_state_size() != C.sizeof(MUState) or lib.espm_mu_abi_version() != ABI_VERSION or theirs != ours:
        raise ImportError(f"{path} was built from another include/espm_mu.h (ABI {lib.espm_mu_abi_version()} / {lib.espm_mu_state_size()} bytes "
                          f"against {ABI_VERSION} / {C.sizeof(MUState)}): rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`")
    return lib


lib = _load()


def last_error(which=None) -> str:
    return (which or lib).espm_mu_last_error().decode()


def check(rc: int, which=None) -> None:
    """Status code -> the exception the reference raises in the same situation."""
    if rc == OK:
        return
    msg = last_error(which)
    if rc == ENOSOLUTION:
        raise ValueError(msg)  # espm/estimators/dicotomy.py:22-23
    if rc == EINVAL:
        raise ValueError(msg)
    if rc == EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise EspmError(msg)


class Variant:
    """One build of the library (include/espm_mu.h): its handle and the sizes that follow its component stride KP."""

    def __init__(self, handle, kp, min_k, max_k):
        self.lib, self.KP, self.MIN_K, self.MAX_K = handle, kp, min_k, max_k
        d = _abi.parse_defines(_HEADER_TEXT, predefined={"ESPM_KP": kp})   # the header as this build's -DESPM_KP compiled it
        self.HP_STRIDE, self.HS_STRIDE, self.HS_MAX = d["ESPM_HP_STRIDE"], d["ESPM_HS_STRIDE"], d["ESPM_HS_MAX"]

    def check(self, rc):
        check(rc, self.lib)


_narrow = Variant(lib, KP, 1, MAX_K)
_wide = None
_widest = None
WIDE_LIB_PATH = os.environ.get("ESPM_MU_WIDE_LIB", os.path.join(_HERE, "lib", "libespm_mu_wide.so"))
WIDEST_LIB_PATH = os.environ.get("ESPM_MU_WIDEST_LIB", os.path.join(_HERE, "lib", "libespm_mu_wide32.so"))


def variant(k) -> Variant:
    """The build that holds the kernels for k components: 1..8 libespm_mu.so, 9..16 libespm_mu_wide.so, 17..32 libespm_mu_wide32.so
    (the dense stores, both contractions on the matrix cores)."""
    global _wide, _widest
    if k <= MAX_K:
        return _narrow
    if k > WIDEST_MAX_K:
        raise NotImplementedError(f"n_components = {k}: the kernels are built for 1..{WIDEST_MAX_K} components")
    if k <= WIDE_MAX_K:
        if _wide is None:
            _wide = Variant(_load(WIDE_LIB_PATH), 16, MAX_K + 1, WIDE_MAX_K)
        return _wide
    if _widest is None:
        _widest = Variant(_load(WIDEST_LIB_PATH), 32, WIDE_MAX_K + 1, WIDEST_MAX_K)
    return _widest

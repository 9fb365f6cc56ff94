"""kmc.py — Python binding of libkmc.so (the C ABI in include/kmc.h).

The product is the HIP/C++ library; this module only marshals pointers for the
tests, the benchmark and Python callers.  Device buffers are torch tensors
(PyTorch is the allocator/stream provider here, nothing else).  There is no CPU
fallback: every entry point raises if libkmc.so is missing or a call fails.

Reference interface mirrored (axlwild/dna-kmeres-parallel):
    sumKmereCoincidencesGlobalMemory(data, indices, num_seqs, sum)  kernels.h:113
        -> dropin_count(data, indices_i32, num_seqs)
    permutationsCountAll generalised to any k, GPU layout           main.cu:636-646
        -> count_dense(data, indices, k)
    importSeqs / importSeqsNoNL                                     main.cu:474-545 / 401-473
        -> load_fasta(path, dialect)

Streams: every device wrapper takes `stream=` (None: torch's current stream) and
hands it to the library.  What the wrapper itself does with tensors (allocating
outputs, zeroing, padding, `.contiguous()` copies) runs on that same stream: with
`stream=s` given it is done under `torch.cuda.stream(s)`, so the library never
reads or writes a tensor the wrapper is still preparing on another stream.  The
caller orders its own use of the inputs and results against `s`.  The wrappers
that return tensors also take `out=`: the caller's own output tensors, in the
order they are returned.
"""
import collections
import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_PATH = os.environ.get("KMC_LIB") or os.path.join(HERE, "lib", "libkmc.so")
# the diagnostic build (test hooks kmc_diag_*, see diag()); never used by the product path
DIAG_LIB_PATH = os.environ.get("KMC_DIAG_LIB") or os.path.join(HERE, "lib", "libkmc_diag.so")
HEADER = os.path.join(REPO, "include", "kmc.h")

DIALECT_BLANK = 0  # importSeqs
DIALECT_NONL = 1   # importSeqsNoNL
MAX_SEQS_REFERENCE = 100
DROPIN_K = 3
KMC_ERR_CAPACITY = 1009
KMC_ERR_RECORD_TOO_LONG = 1010
KMC_ERR_INTERNAL = 1011
KMC_ERR_FORMAT = 1012
KMC_FASTQ_KEEP_RAW = 1


class KmcError(RuntimeError):
    """`record`: with KMC_ERR_FORMAT the 0-based index of the malformed record, else None."""

    def __init__(self, code, what, record=None):
        self.code = code
        self.record = record
        at = " at record %d" % record if record is not None else ""
        super().__init__("%s failed: %s%s (%d)" % (what, error_string(code), at, code))


_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
_I64 = ctypes.c_int64


class DenseArgs(ctypes.Structure):
    _fields_ = [
        ("data", _P), ("indices", _P), ("num_seqs", _U64), ("k", ctypes.c_int),
        ("sum", _P), ("sum_ld", _U64), ("invalid", _P),
        ("read_lo", _U64), ("read_hi", _U64), ("win_lo", _U64), ("win_hi", _U64),
        ("workspace", _P), ("workspace_bytes", ctypes.c_size_t), ("status", _P),
    ]


class SpectrumSummary(ctypes.Structure):
    _fields_ = [
        ("scale", ctypes.c_double), ("sampled_distinct", _U64), ("sampled_total", _U64),
        ("distinct", ctypes.c_double), ("total", ctypes.c_double),
        ("valley", ctypes.c_uint32), ("peak", ctypes.c_uint32), ("min_abundance", ctypes.c_uint32),
        ("saturated", ctypes.c_uint32), ("genome_size", ctypes.c_double),
    ]


class SketchLink(ctypes.Structure):
    """kmc_sketch_link: one listed pair of kmc_sketch_links[_rect], 16 bytes."""
    _fields_ = [("i", ctypes.c_uint32), ("j", ctypes.c_uint32), ("shared", ctypes.c_uint32), ("denom", ctypes.c_uint32)]


_lib = None
_diag_lib = None
_active = None  # the diagnostic library while inside diag()


def lib():
    """Load libkmc.so (built in-tree by `make -C dna-kmeres-parallel_amd`)."""
    global _lib
    if _active is not None:
        return _active
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


class diag:
    """Context manager: inside it every binding calls lib/libkmc_diag.so, the same
    library built with the test hooks (kmc_diag_radix_mode, kmc_diag_canon_claim_cap,
    kmc_diag_canon_sort_cap, kmc_diag_dense_spill_cap) that force an algorithm
    choice (kmc_diag_canon_sort_cap_big, kmc_diag_canon_direct too); libkmc.so
    exports none of them.  `with kmc.diag() as D: D.kmc_diag_...`"""

    def __enter__(self):
        global _diag_lib, _active
        if _diag_lib is None:
            _diag_lib = _load(DIAG_LIB_PATH)
            _diag_lib.kmc_diag_radix_mode.argtypes = [ctypes.c_int, ctypes.c_float]
            _diag_lib.kmc_diag_canon_claim_cap.argtypes = [ctypes.c_uint]
            _diag_lib.kmc_diag_canon_sort_cap.argtypes = [ctypes.c_uint]
            _diag_lib.kmc_diag_canon_sort_cap_big.argtypes = [ctypes.c_uint]
            _diag_lib.kmc_diag_canon_direct.argtypes = [ctypes.c_int]
            _diag_lib.kmc_diag_canon_fallback.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)] * 2
            _diag_lib.kmc_diag_canon_fallback_detail.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_uint,
                                                                 ctypes.POINTER(ctypes.c_ulonglong)]
            _diag_lib.kmc_diag_dense_spill_cap.argtypes = [ctypes.c_uint]
            _diag_lib.kmc_diag_canon_stale_queue.argtypes = [ctypes.c_longlong]
            _diag_lib.kmc_diag_canon_list_target.argtypes = [ctypes.c_uint]
        self._prev = _active
        _active = _diag_lib
        return _diag_lib

    def __exit__(self, *exc):
        global _active
        L = _active
        # restore the defaults for the next user of the diagnostic library
        L.kmc_diag_radix_mode(0, 1.0)
        L.kmc_diag_canon_claim_cap(0)
        L.kmc_diag_canon_sort_cap(1 << 30)  # (also restores the big instance's cap)
        L.kmc_diag_canon_direct(1)
        L.kmc_diag_dense_spill_cap(0)
        L.kmc_diag_canon_stale_queue(-1)
        L.kmc_diag_canon_list_target(0)
        _active = self._prev
        return False


def hip_runtimes():
    """Paths of the HIP runtime libraries (libamdhip64) mapped into this process."""
    with open("/proc/self/maps") as f:
        return sorted(set(line.split()[-1] for line in f if "/libamdhip64.so" in line))


def _load(path):
    """One HIP runtime per process: torch ships its own libamdhip64 (torch/lib),
    libkmc.so names the SONAME libamdhip64.so.7 (found through its RUNPATH in
    /opt/rocm/lib).  The dynamic loader satisfies a NEEDED entry with an already
    loaded library of that SONAME, so torch is imported FIRST (when it is
    installed) and libkmc then binds to torch's runtime; loaded the other way
    round, both runtimes would be mapped and each would initialise the GPU on its
    own.  A second runtime mapped anyway is refused here."""
    if not os.path.exists(path):
        raise RuntimeError("%s not built: run `make -C %s` (no CPU fallback exists)" % (os.path.basename(path), HERE))
    # KMC_NO_TORCH=1: host-only use of the binding (loader, shard planner) without
    # paying torch's import; such a process must then not import torch at all
    if os.environ.get("KMC_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401  (maps torch's HIP runtime before libkmc's NEEDED entry is resolved)
        except ImportError:
            pass
    L = ctypes.CDLL(path)
    rt = hip_runtimes()
    if len(rt) > 1:
        raise RuntimeError("two HIP runtimes are mapped in this process (%s): each would initialise the GPU on its "
                           "own, so %s is refused; import torch before loading it (or set KMC_NO_TORCH=1 only in "
                           "processes that never import torch)" % (", ".join(rt), os.path.basename(path)))
    L.kmc_error_string.restype = ctypes.c_char_p
    L.kmc_error_string.argtypes = [ctypes.c_int]
    L.kmc_version.restype = ctypes.c_int
    L.kmc_version.argtypes = []
    L.sumKmereCoincidencesGlobalMemory_hip.argtypes = [_P, _P, ctypes.c_uint, _P, _P]
    L.kmc_count_dense_workspace_size.restype = ctypes.c_size_t
    L.kmc_count_dense_workspace_size.argtypes = [ctypes.c_int, _U64, _U64, ctypes.c_int]
    L.kmc_count_dense.argtypes = [_P, _P, _U64, _U64, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_count_dense_ex.argtypes = [ctypes.POINTER(DenseArgs), _P]
    L.kmc_count_dense_ex_workspace_size.restype = ctypes.c_size_t
    L.kmc_count_dense_ex_workspace_size.argtypes = [ctypes.POINTER(DenseArgs), ctypes.c_int]
    L.kmc_dense_status.argtypes = [ctypes.c_int]
    L.kmc_trace_set_events.argtypes = [_P, _P]
    L.kmc_set_reserved_cus.argtypes = [ctypes.c_int]
    L.kmc_plan_shards.argtypes = [_P, _U64, ctypes.c_int, ctypes.c_int, _U64, _P]
    L.kmc_count_multi.argtypes = [_P, _P, _U64, _U64, ctypes.c_int, ctypes.c_int, _P, _P, _P]
    L.kmc_multi_release.argtypes = []
    L.kmc_synth_fill.argtypes = [_P, _U64, _U64, _U64, _U64, _P]
    L.kmc_synth_fill_range.argtypes = [_P, _U64, _U64, _U64, _U64, _P]
    L.kmc_synth_indices.argtypes = [_P, _U64, _U64]
    L.kmc_synth_indices.restype = None
    L.kmc_fasta_load.argtypes = [ctypes.c_char_p, ctypes.c_int, _I64, ctypes.POINTER(_P)]
    for fn in ("kmc_fasta_num_seqs", "kmc_fasta_data_bytes", "kmc_fasta_reference_num_indexes"):
        getattr(L, fn).restype = _U64
        getattr(L, fn).argtypes = [_P]
    L.kmc_fasta_indices.restype = _P
    L.kmc_fasta_indices.argtypes = [_P]
    L.kmc_fasta_data.restype = _P
    L.kmc_fasta_data.argtypes = [_P]
    L.kmc_fasta_free.argtypes = [_P]
    L.kmc_fasta_free.restype = None
    L.kmc_fasta_parse_device.argtypes = [_P, _U64, ctypes.c_int, _P, _U64, _P, _U64, ctypes.POINTER(_U64),
                                         ctypes.POINTER(_U64), _P]
    L.kmc_fasta_load_device.argtypes = [ctypes.c_char_p, ctypes.c_int, _I64, ctypes.POINTER(_P),
                                        ctypes.POINTER(_U64), ctypes.POINTER(_P), ctypes.POINTER(_U64), _P]
    L.kmc_fastq_parse_device.argtypes = [_P, _U64, ctypes.c_int, _P, _U64, _P, _U64, ctypes.POINTER(_U64),
                                         ctypes.POINTER(_U64), ctypes.POINTER(_U64), _P]
    L.kmc_fastq_load_device.argtypes = [ctypes.c_char_p, _I64, ctypes.POINTER(_P), ctypes.POINTER(_U64),
                                        ctypes.POINTER(_P), ctypes.POINTER(_U64), _P]
    L.kmc_fastq_open.argtypes = [ctypes.c_char_p, _U64, ctypes.POINTER(_P)]
    L.kmc_fastq_next.argtypes = [_P, ctypes.POINTER(_P), ctypes.POINTER(_U64), ctypes.POINTER(_P),
                                 ctypes.POINTER(_U64), _P]
    L.kmc_fastq_close.argtypes = [_P]
    L.kmc_fastq_parse_device_ex.argtypes = [_P, _U64, ctypes.c_int, _P, _U64, _P, _U64, ctypes.POINTER(_U64),
                                            ctypes.POINTER(_U64), ctypes.POINTER(_U64), _P, _P]
    L.kmc_fastq_open_ex.argtypes = [ctypes.c_char_p, _U64, ctypes.c_uint, ctypes.POINTER(_P)]
    L.kmc_fastq_raw.argtypes = [_P, ctypes.POINTER(_P), ctypes.POINTER(_U64), ctypes.POINTER(_P)]
    L.kmc_select_records_workspace_size.restype = ctypes.c_size_t
    L.kmc_select_records_workspace_size.argtypes = [_U64, _U64]
    L.kmc_select_records.argtypes = [_P, _P, _U64, _U64, _P, ctypes.c_int, _P, _U64, _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_match_select.argtypes = [_P, _P, _U64, ctypes.c_uint32, ctypes.c_double, _P, _P, _P]
    L.kmc_fastq_close.restype = None
    L.kmc_pair_distances_workspace_size.restype = ctypes.c_size_t
    L.kmc_pair_distances_workspace_size.argtypes = [_U64, ctypes.c_int, ctypes.c_int]
    L.kmc_pair_distances.argtypes = [_P, _U64, _P, _U64, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]
    L.kmc_pair_distances_sparse_workspace_size.restype = ctypes.c_size_t
    L.kmc_pair_distances_sparse_workspace_size.argtypes = [_U64, _U64, ctypes.c_int]
    L.kmc_pair_distances_sparse.argtypes = [_P, _P, _P, _U64, _P, _U64, ctypes.c_int, _P, _P, ctypes.c_size_t, _P]
    L.kmc_sketch_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_workspace_size.argtypes = [_U64, _U64, ctypes.c_uint32, ctypes.c_int]
    L.kmc_sketch_from_counts.argtypes = [_P, _P, _P, _U64, _U64, ctypes.c_uint32, _U64, ctypes.c_uint32, _P, _P, _P,
                                         ctypes.c_size_t, _P]
    L.kmc_sketch_distances.argtypes = [_P, _P, _U64, ctypes.c_uint32, ctypes.c_int, _P, _P, _P, _P]
    L.kmc_sketch_from_sequences_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_from_sequences_workspace_size.argtypes = [_U64, _U64, ctypes.c_uint32, ctypes.c_int]
    L.kmc_sketch_from_sequences.argtypes = [_P, _P, _U64, _U64, ctypes.c_int, ctypes.c_uint, ctypes.c_uint32, _U64,
                                            _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_sketch_from_sequences_grouped_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_from_sequences_grouped_workspace_size.argtypes = [_U64, _U64, _U64, ctypes.c_uint32, ctypes.c_int]
    L.kmc_sketch_from_sequences_grouped.argtypes = [_P, _P, _U64, _U64, _P, _U64, ctypes.c_int, ctypes.c_uint,
                                                    ctypes.c_uint32, _U64, _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_sketch_merge_groups.argtypes = [_P, _P, _U64, _P, _U64, ctypes.c_uint32, _P, _P, _P]
    L.kmc_sketch_distances_rect.argtypes = [_P, _P, _U64, _P, _P, _U64, ctypes.c_uint32, ctypes.c_int, _P, _P, _P, _P]
    L.kmc_sketch_nearest_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_nearest_workspace_size.argtypes = [_U64, _U64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    L.kmc_sketch_nearest.argtypes = [_P, _P, _U64, _P, _P, _U64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32,
                                     ctypes.c_uint32, _P, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_mash_jaccard_of_distance.restype = ctypes.c_double
    L.kmc_mash_jaccard_of_distance.argtypes = [ctypes.c_double, ctypes.c_int]
    L.kmc_sketch_cluster_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_cluster_workspace_size.argtypes = [_U64, ctypes.c_int]
    L.kmc_sketch_cluster.argtypes = [_P, _P, _U64, ctypes.c_uint32, ctypes.c_double, _P, _P, _P, _P, ctypes.c_size_t,
                                     _P]
    L.kmc_sketch_links.argtypes = [_P, _P, _U64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, _P, _P, _U64, _P, _P]
    L.kmc_sketch_links_rect.argtypes = [_P, _P, _U64, _P, _P, _U64, ctypes.c_uint32, ctypes.c_int, ctypes.c_double, _P,
                                        _P, _U64, _P, _P]
    L.kmc_sketch_screen_index_size.restype = ctypes.c_size_t
    L.kmc_sketch_screen_index_size.argtypes = [_U64, ctypes.c_uint32]
    L.kmc_sketch_screen_build.argtypes = [_P, _P, _U64, ctypes.c_uint32, _P, ctypes.c_size_t, _P]
    L.kmc_sketch_screen_count.argtypes = [_P, ctypes.c_size_t, _P, _P, _U64, _U64, ctypes.c_int, ctypes.c_uint, _U64, _P]
    L.kmc_sketch_screen_results.argtypes = [_P, ctypes.c_size_t, _P, _P, _U64, ctypes.c_uint32, ctypes.c_int, _P, _P,
                                            _P, _P]
    L.kmc_sketch_screen_winners_workspace_size.restype = ctypes.c_size_t
    L.kmc_sketch_screen_winners_workspace_size.argtypes = [ctypes.c_size_t, _U64]
    L.kmc_sketch_screen_winners.argtypes = [_P, ctypes.c_size_t, _P, _P, _U64, ctypes.c_uint32, ctypes.c_int, _P, _P,
                                            _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_sketch_accum_device_bytes.restype = ctypes.c_size_t
    L.kmc_sketch_accum_device_bytes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.kmc_sketch_accum_create.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint, _U64, ctypes.c_uint32,
                                          ctypes.POINTER(_P)]
    L.kmc_sketch_accum_add.argtypes = [_P, _P, _P, _U64, _U64, _P]
    L.kmc_sketch_accum_finish.argtypes = [_P, ctypes.c_uint32, _P, _P, _P, _P]
    L.kmc_sketch_accum_reset.argtypes = [_P, _P]
    L.kmc_sketch_accum_free.argtypes = [_P]
    L.kmc_sketch_accum_free.restype = None
    L.kmc_spectrum_from_accum.argtypes = [_P, ctypes.c_uint32, _P, _P, _P]
    L.kmc_match_from_accum.argtypes = [_P, _P, _P, _U64, _U64, ctypes.c_uint32, _P, _P, _P, _P, _P]
    L.kmc_label_accum.argtypes = [_P, _P, _P, _U64, _U64, ctypes.c_uint32, _P]
    L.kmc_classify_workspace_size.restype = ctypes.c_size_t
    L.kmc_classify_workspace_size.argtypes = [_U64, _U64, ctypes.c_uint32, ctypes.c_int]
    L.kmc_classify_from_accum.argtypes = [_P, _P, _P, _U64, _U64, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P, _P, _P,
                                          _P, _P, _P, _P, ctypes.c_size_t, _P]
    L.kmc_classify_select.argtypes = [_P, _P, _P, _P, _U64, ctypes.c_uint32, ctypes.c_uint32, _P, _P, _P]
    L.kmc_spectrum_summarize.argtypes = [_P, ctypes.c_uint32, _U64, ctypes.POINTER(SpectrumSummary)]
    L.minKmeres2_hip.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P, _P]
    L.kmc_count_canonical_hash.argtypes = [_P, _P, _U64, ctypes.c_int, ctypes.c_uint, _P, _P, _U64, _P,
                                           ctypes.POINTER(_U64), _P]
    L.kmc_count_canonical_hash_ex.argtypes = [_P, _P, _U64, ctypes.c_int, ctypes.c_uint, _P, _P, _U64, _P,
                                              ctypes.POINTER(_U64), _P, ctypes.c_size_t, _P]
    L.kmc_count_canonical_workspace_size.restype = ctypes.c_size_t
    L.kmc_count_canonical_workspace_size.argtypes = [_P, _U64, ctypes.c_int, ctypes.c_int]
    return L


def error_string(code):
    return lib().kmc_error_string(int(code)).decode()


def _check(rc, what, record=None):
    if rc != 0:
        raise KmcError(rc, what, int(record) if rc == KMC_ERR_FORMAT and record is not None else None)


def header_symbols(path=HEADER):
    """Function names declared by include/kmc.h."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"^[A-Za-z_][\w \*]*?\b(\w+)\s*\(", txt, flags=re.M)
    return sorted(set(n for n in names if n not in ("defined",)))


# ---------------------------------------------------------------------------
# device entry points (torch tensors on cuda)
# ---------------------------------------------------------------------------
def _stream(stream):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _on(stream):
    """Context of a wrapper's own tensor work: on `stream` when one is given, else
    on the current stream (see the module docstring)."""
    import torch
    return torch.cuda.stream(stream)  # (a no-op for None)


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ws(workspace):
    """(pointer, bytes) of a caller's workspace tensor; None: (None, 0), the library's own."""
    if workspace is None:
        return None, 0
    return _dptr(workspace), workspace.numel() * workspace.element_size()


def _sketch_out(n, s, device, out=None):
    """Uninitialised (sketches int64 [n, s], sizes int32 [n]) of the sketch entry
    points, or the caller's own pair `out`."""
    import torch
    if out is not None:
        return out
    return (torch.empty((max(n, 0), max(s, 0)), dtype=torch.int64, device=device),
            torch.empty(max(n, 0), dtype=torch.int32, device=device))


def dropin_count(data, indices, num_seqs=None, out=None, stream=None):
    """Exact drop-in of the reference launch (k = 3): returns int32 sum[4^3 * n]
    in the reference layout sum[s + n*code] (flat, like the reference)."""
    import torch
    n = int(num_seqs if num_seqs is not None else indices.numel() - 1)
    if out is None:
        with _on(stream):
            out = torch.empty((1 << (2 * DROPIN_K)) * n, dtype=torch.int32, device=data.device)
    rc = lib().sumKmereCoincidencesGlobalMemory_hip(_dptr(data), _dptr(indices), n, _dptr(out), _stream(stream))
    _check(rc, "sumKmereCoincidencesGlobalMemory_hip")
    return out


def dense_workspace_size(k, num_seqs, data_bytes, device=0):
    return int(lib().kmc_count_dense_workspace_size(k, num_seqs, data_bytes, device))


def count_dense(data, indices, k, data_bytes=None, invalid=False, workspace=None, out=None, stream=None):
    """k-mer histogram of every record: returns (sum (4^k, n) int32, invalid (n,) or None).
    `invalid`: True for a new tensor, or the caller's own int32 tensor (n,)."""
    import torch
    n = indices.numel() - 1
    nb = 1 << (2 * k)
    if data_bytes is None:
        data_bytes = data.numel()
    with _on(stream):
        if out is None:
            out = torch.empty((nb, n), dtype=torch.int32, device=data.device)
        if isinstance(invalid, torch.Tensor):
            inv = invalid
        else:
            inv = torch.empty(n, dtype=torch.int32, device=data.device) if invalid else None
    rc = lib().kmc_count_dense(_dptr(data), _dptr(indices), n, data_bytes, k, _dptr(out), _dptr(inv),
                               *_ws(workspace), _stream(stream))
    _check(rc, "kmc_count_dense")
    return out, inv


def dense_args(data, indices, k, out, read=(0, None), win=(0, None), ld=0, invalid=None, workspace=None,
               data_offset=0, status=None):
    """Build a kmc_dense_args.  `data_offset` = global offset of data[0] (the data
    pointer handed to the library is data_ptr - data_offset).  `status`: an int32
    device tensor (zeroed by the caller) that receives this call's deferred status
    (see dense_status_check); None: the device's flag (kmc_dense_status)."""
    a = DenseArgs()
    a.data = ctypes.c_void_p(data.data_ptr() - data_offset)
    a.indices = ctypes.c_void_p(indices.data_ptr())
    a.num_seqs = indices.numel() - 1
    a.k = k
    a.sum = ctypes.c_void_p(out.data_ptr())
    a.sum_ld = ld
    a.invalid = _dptr(invalid)
    a.read_lo = read[0]
    a.read_hi = read[1] if read[1] is not None else data_offset + data.numel()
    a.win_lo = win[0]
    a.win_hi = win[1] if win[1] is not None else data_offset + data.numel()
    a.workspace, a.workspace_bytes = _ws(workspace)
    a.status = _dptr(status)
    return a


def dense_status_check(status=None, device=None):
    """Raise KmcError for a failed asynchronous dense call (synchronises first):
    `status` = the call's own int32 status tensor, or None for the device's flag
    (kmc_dense_status, which it clears)."""
    import torch
    torch.cuda.synchronize()
    if status is not None:
        _check(int(status.reshape(-1)[0].item()), "dense count (deferred status)")
    else:
        dv = torch.cuda.current_device() if device is None else device
        _check(lib().kmc_dense_status(dv), "dense count (kmc_dense_status)")


def count_dense_ex(args, stream=None):
    rc = lib().kmc_count_dense_ex(ctypes.byref(args), _stream(stream))
    _check(rc, "kmc_count_dense_ex")


def dense_ex_workspace_size(args, device=0):
    return int(lib().kmc_count_dense_ex_workspace_size(ctypes.byref(args), device))


def pair_distances_workspace_size(num_seqs, k, device=0):
    return int(lib().kmc_pair_distances_workspace_size(num_seqs, k, device))


def pair_distances(counts, indices, k, num_seqs=None, ld=0, out=None, workspace=None, stream=None):
    """All-pairs k-mer distance (kmc_pair_distances): `counts` is the int32 count
    matrix sum[s + ld*code] (e.g. count_dense's (4^k, n) tensor), `indices` the
    device int64 offsets.  Returns float32 [n(n-1)/2], packed upper triangle."""
    import torch
    n = int(num_seqs if num_seqs is not None else indices.numel() - 1)
    if out is None:
        with _on(stream):
            out = torch.empty(max(n * (n - 1) // 2, 0), dtype=torch.float32, device=counts.device)
    rc = lib().kmc_pair_distances(_dptr(counts), ld, _dptr(indices), n, k, _dptr(out), *_ws(workspace),
                                  _stream(stream))
    _check(rc, "kmc_pair_distances")
    return out


CANON_SOFTMASK = 1
CANON_FORWARD = 2
CANON_MAX_K = 31


def count_canonical(data, indices, k, flags=0, capacity=None, workspace=None, out=None, stream=None):
    """Canonical k-mer counts per record (kmc_count_canonical_hash[_ex]): returns
    (keys uint64 as int64 tensor, counts int32 tensor, rec_offsets int64 tensor);
    record s owns [rec_offsets[s], rec_offsets[s+1]), order within it unspecified.
    `workspace`: a caller device buffer of canonical_workspace_size() bytes (None:
    the library's own).  `out`: the caller's own (keys, counts, rec_offsets), the
    first two of `capacity` elements; views of them are returned."""
    import torch
    n = indices.numel() - 1
    if capacity is None:
        capacity = max(int(data.numel()), 1)
    if out is not None:
        keys, counts, off = out
    else:
        with _on(stream):
            keys = torch.empty(capacity, dtype=torch.int64, device=data.device)
            counts = torch.empty(capacity, dtype=torch.int32, device=data.device)
            off = torch.zeros(max(n + 1, 1), dtype=torch.int64, device=data.device)
    tot = _U64(0)
    # (kmc_count_canonical_hash is this call with no workspace)
    rc = lib().kmc_count_canonical_hash_ex(_dptr(data), _dptr(indices), n, k, flags, _dptr(keys), _dptr(counts),
                                           capacity, _dptr(off), ctypes.byref(tot), *_ws(workspace), _stream(stream))
    _check(rc, "kmc_count_canonical_hash")
    t = int(tot.value)
    return keys[:t], counts[:t], off


def canonical_workspace_size(indices_host, k, device=0):
    """kmc_count_canonical_workspace_size for host int64 offsets (num_seqs + 1)."""
    idx = np.ascontiguousarray(indices_host, dtype=np.int64)
    return int(lib().kmc_count_canonical_workspace_size(idx.ctypes.data_as(_P), idx.size - 1, k, device))


def pair_distances_sparse_workspace_size(num_seqs, num_entries, device=0):
    return int(lib().kmc_pair_distances_sparse_workspace_size(num_seqs, num_entries, device))


def pair_distances_sparse(keys, counts, rec_offsets, indices, k, num_entries=None, out=None, workspace=None,
                          stream=None):
    """All-pairs k-mer distance from per-record (key, count) lists
    (kmc_pair_distances_sparse): `keys` (64-bit), `counts` (32-bit) and `rec_offsets`
    (64-bit, n + 1) as count_canonical returns them, `indices` the device int64
    record offsets.  Returns float32 [n(n-1)/2], packed upper triangle."""
    import torch
    n = int(indices.numel() - 1)
    if num_entries is None:
        num_entries = keys.numel()
    if out is None:
        with _on(stream):
            out = torch.empty(max(n * (n - 1) // 2, 0), dtype=torch.float32, device=indices.device)
    rc = lib().kmc_pair_distances_sparse(_dptr(keys), _dptr(counts), _dptr(rec_offsets), int(num_entries),
                                         _dptr(indices), n, k, _dptr(out), *_ws(workspace), _stream(stream))
    _check(rc, "kmc_pair_distances_sparse")
    return out


SKETCH_MAX_SIZE = 16384
SKETCH_DEFAULT_SEED = 42


def sketch_workspace_size(num_seqs, num_entries, sketch_size, device=0):
    return int(lib().kmc_sketch_workspace_size(num_seqs, num_entries, sketch_size, device))


def sketch_from_counts(keys, counts, rec_offsets, sketch_size, seed=SKETCH_DEFAULT_SEED, min_count=1,
                       workspace=None, num_entries=None, out=None, stream=None):
    """Bottom-s MinHash sketches (kmc_sketch_from_counts) of per-record lists as
    count_canonical returns them (`counts` may be None while min_count <= 1).
    Returns (sketches int64 [n, s]: uint64 hashes ascending, then all-ones fill;
    sizes int32 [n])."""
    n = int(rec_offsets.numel() - 1)
    s = int(sketch_size)
    if num_entries is None:
        num_entries = keys.numel()
    with _on(stream):
        sk, sizes = _sketch_out(n, s, rec_offsets.device, out)
    rc = lib().kmc_sketch_from_counts(_dptr(keys), _dptr(counts), _dptr(rec_offsets), int(num_entries), n, s,
                                      int(seed) & _M64, int(min_count), _dptr(sk), _dptr(sizes), *_ws(workspace),
                                      _stream(stream))
    _check(rc, "kmc_sketch_from_counts")
    return sk, sizes


def sketch_from_sequences_workspace_size(num_seqs, data_bytes, sketch_size, device=0):
    return int(lib().kmc_sketch_from_sequences_workspace_size(num_seqs, data_bytes, sketch_size, device))


def sketch_from_sequences(data, indices, k, sketch_size, flags=0, seed=SKETCH_DEFAULT_SEED, data_bytes=None,
                          workspace=None, out=None, stream=None):
    """Bottom-s MinHash sketches straight from the record buffer
    (kmc_sketch_from_sequences): the rows and sizes sketch_from_counts gives for
    count_canonical's lists of the same data, indices, k and flags, in one pass and
    without those lists.  Returns (sketches int64 [n, s], sizes int32 [n])."""
    n = int(indices.numel() - 1)
    s = int(sketch_size)
    if data_bytes is None:
        data_bytes = data.numel()
    with _on(stream):
        sk, sizes = _sketch_out(n, s, indices.device, out)
    rc = lib().kmc_sketch_from_sequences(_dptr(data), _dptr(indices), n, int(data_bytes), k, flags, s,
                                         int(seed) & _M64, _dptr(sk), _dptr(sizes), *_ws(workspace),
                                         _stream(stream))
    _check(rc, "kmc_sketch_from_sequences")
    return sk, sizes


def sketch_from_sequences_grouped_workspace_size(num_seqs, num_groups, data_bytes, sketch_size, device=0):
    return int(lib().kmc_sketch_from_sequences_grouped_workspace_size(num_seqs, num_groups, data_bytes, sketch_size,
                                                                      device))


def sketch_from_sequences_grouped(data, indices, group_offsets, k, sketch_size, flags=0, seed=SKETCH_DEFAULT_SEED,
                                  data_bytes=None, workspace=None, out=None, stream=None):
    """One bottom-s MinHash sketch per group of consecutive records
    (kmc_sketch_from_sequences_grouped): group g owns the records
    [group_offsets[g], group_offsets[g+1]) (device int64 tensor) and its row is the
    sketch of the union of their k-mer sets.  Returns (sketches int64 [groups, s],
    sizes int32 [groups]); without a record every group is empty (size 0, fill)."""
    n = int(indices.numel() - 1)
    ng = int(group_offsets.numel() - 1)
    s = int(sketch_size)
    if data_bytes is None:
        data_bytes = data.numel()
    with _on(stream):
        sk, sizes = _sketch_out(ng, s, indices.device, out)
    rc = lib().kmc_sketch_from_sequences_grouped(_dptr(data), _dptr(indices), n, int(data_bytes),
                                                 _dptr(group_offsets), ng, k, flags, s, int(seed) & _M64, _dptr(sk),
                                                 _dptr(sizes), *_ws(workspace), _stream(stream))
    _check(rc, "kmc_sketch_from_sequences_grouped")
    if n <= 0:  # the library writes nothing then
        with _on(stream):
            sk.fill_(-1)
            sizes.zero_()
    return sk, sizes


def sketch_merge_groups(sketches, sizes, group_offsets, out=None, stream=None):
    """Bottom-s of the union of the sketch rows [group_offsets[g], group_offsets[g+1])
    (kmc_sketch_merge_groups) for every group g.  Returns new (sketches int64
    [groups, s], sizes int32 [groups]); the input is left as it is."""
    with _on(stream):
        sketches = sketches.contiguous()
    rows, s = int(sketches.shape[0]), int(sketches.shape[1])
    ng = int(group_offsets.numel() - 1)
    with _on(stream):
        sk, sz = _sketch_out(ng, s, sketches.device, out)
    rc = lib().kmc_sketch_merge_groups(_dptr(sketches), _dptr(sizes), rows, _dptr(group_offsets), ng, s, _dptr(sk),
                                       _dptr(sz), _stream(stream))
    _check(rc, "kmc_sketch_merge_groups")
    return sk, sz


def _dist_out(shape, device, with_counts, out):
    """Uninitialised (out float32, shared, denom int32 or None, None) of `shape`, or
    the caller's own triple `out`."""
    import torch
    if out is not None:
        return out
    return (torch.empty(shape, dtype=torch.float32, device=device),
            torch.empty(shape, dtype=torch.int32, device=device) if with_counts else None,
            torch.empty(shape, dtype=torch.int32, device=device) if with_counts else None)


def sketch_distances(sketches, sizes, k, with_counts=False, out=None, stream=None):
    """All-pairs Mash distance (kmc_sketch_distances) of sketch rows [n, s] and their
    sizes [n].  Returns float32 [n(n-1)/2], packed upper triangle; with_counts:
    (out, shared, denom), the two integer counts as int32 tensors."""
    with _on(stream):
        sketches = sketches.contiguous()
        n, s = int(sketches.shape[0]), int(sketches.shape[1])
        out, sh, dn = _dist_out(max(n * (n - 1) // 2, 0), sketches.device, with_counts, out)
    rc = lib().kmc_sketch_distances(_dptr(sketches), _dptr(sizes), n, s, k, _dptr(out), _dptr(sh), _dptr(dn),
                                    _stream(stream))
    _check(rc, "kmc_sketch_distances")
    return (out, sh, dn) if with_counts else out


NEAREST_MAX_TOP = 1024


def _row_sets(q, r, stream):
    """Contiguous query and reference rows of one sketch size: (q, r, m, n, s)."""
    with _on(stream):
        q, r = q.contiguous(), r.contiguous()
    if int(q.shape[1]) != int(r.shape[1]):
        raise ValueError("query rows of %d values against reference rows of %d" % (q.shape[1], r.shape[1]))
    return q, r, int(q.shape[0]), int(r.shape[0]), int(q.shape[1])


def sketch_distances_rect(q, qs, r, rs, k, with_counts=False, out=None, stream=None):
    """Mash distance of every query row against every reference row
    (kmc_sketch_distances_rect): rows q [m, s] with sizes qs [m], rows r [n, s] with
    sizes rs [n].  Returns float32 [m, n]; with_counts: (out, shared, denom), the
    two integer counts as int32 tensors [m, n]."""
    q, r, m, n, s = _row_sets(q, r, stream)
    with _on(stream):
        out, sh, dn = _dist_out((m, n), q.device, with_counts, out)
    rc = lib().kmc_sketch_distances_rect(_dptr(q), _dptr(qs), m, _dptr(r), _dptr(rs), n, s, k, _dptr(out), _dptr(sh),
                                         _dptr(dn), _stream(stream))
    _check(rc, "kmc_sketch_distances_rect")
    return (out, sh, dn) if with_counts else out


def sketch_nearest_workspace_size(num_queries, num_refs, sketch_size, top, device=0):
    return int(lib().kmc_sketch_nearest_workspace_size(num_queries, num_refs, sketch_size, top, device))


def sketch_nearest(q, qs, r, rs, k, top, min_shared=1, workspace=None, out=None, stream=None):
    """The `top` nearest reference rows of every query row (kmc_sketch_nearest), by
    Jaccard estimate shared / denom descending, then by reference index; a
    reference takes part with denom > 0 and shared >= min_shared.  Returns (refs,
    shared, denom int32 [m, top], dist float32 [m, top], counts int32 [m]): row q
    holds counts[q] hits, then -1 (UINT32_MAX), 0, 0 and NaN."""
    import torch
    q, r, m, n, s = _row_sets(q, r, stream)
    top = int(top)
    shape = (m, max(top, 0))
    if out is not None:
        refs, sh, dn, dist, counts = out
    else:
        with _on(stream):
            refs = torch.empty(shape, dtype=torch.int32, device=q.device)
            sh = torch.empty(shape, dtype=torch.int32, device=q.device)
            dn = torch.empty(shape, dtype=torch.int32, device=q.device)
            dist = torch.empty(shape, dtype=torch.float32, device=q.device)
            counts = torch.empty(m, dtype=torch.int32, device=q.device)
    rc = lib().kmc_sketch_nearest(_dptr(q), _dptr(qs), m, _dptr(r), _dptr(rs), n, s, k, top, int(min_shared),
                                  _dptr(refs), _dptr(sh), _dptr(dn), _dptr(dist), _dptr(counts), *_ws(workspace),
                                  _stream(stream))
    _check(rc, "kmc_sketch_nearest")
    return refs, sh, dn, dist, counts


def mash_jaccard_of_distance(d, k):
    """The Jaccard threshold of a Mash distance d at k-mer length k
    (kmc_mash_jaccard_of_distance): e^(-k d) / (2 - e^(-k d)); NaN for a bad d or k."""
    return float(lib().kmc_mash_jaccard_of_distance(float(d), int(k)))


def sketch_cluster_workspace_size(num_seqs, device=0):
    return int(lib().kmc_sketch_cluster_workspace_size(num_seqs, device))


def sketch_cluster(sketches, sizes, min_jaccard, index=True, workspace=None, out=None, stream=None):
    """Single-linkage clusters of sketch rows [n, s] with sizes [n] (kmc_sketch_cluster):
    rows i and j are linked iff denom > 0 and shared >= min_jaccard * denom.  Returns
    (labels int32 [n], cluster_index int32 [n], num_clusters int32 [1]): the smallest
    index of each row's cluster, the cluster's rank by that index, and the number of
    clusters; index=False: (labels, None, None), no ranking.  `out` is the caller's
    own triple, whose second and third entries may be None."""
    import torch
    with _on(stream):
        sketches = sketches.contiguous()
        n, s = int(sketches.shape[0]), int(sketches.shape[1])
        if out is not None:
            labels, cidx, count = out
        else:
            dev = sketches.device
            labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)  # (no row: still a pointer to pass)
            cidx = torch.empty(n, dtype=torch.int32, device=dev) if index else None
            count = torch.empty(1, dtype=torch.int32, device=dev) if index else None
    rc = lib().kmc_sketch_cluster(_dptr(sketches), _dptr(sizes), n, s, float(min_jaccard), _dptr(labels), _dptr(cidx),
                                  _dptr(count), *_ws(workspace), _stream(stream))
    _check(rc, "kmc_sketch_cluster")
    return labels[:n], cidx, count


def _links(call, what, device, capacity, with_dist, out, stream):
    """The two forms of sketch_links / sketch_links_rect: call(links, dist, capacity,
    count) makes the library call on `stream`."""
    import torch

    def make(cap):
        return (torch.empty((cap, 4), dtype=torch.int32, device=device),
                torch.empty(cap, dtype=torch.float32, device=device) if with_dist else None)

    if capacity is not None:
        capacity = int(capacity)
        with _on(stream):
            if out is not None:
                links, dist, count = out
            else:
                links, dist = make(capacity)
                count = torch.empty(1, dtype=torch.int64, device=device)
        _check(call(links if capacity > 0 else None, dist if capacity > 0 else None, capacity, count), what)
        return links, dist, count
    with _on(stream):
        count = out[2] if out is not None else torch.empty(1, dtype=torch.int64, device=device)
        _check(call(None, None, 0, count), what)
        total = int(count.item())  # (waits for the stream)
        links, dist = (out[0], out[1]) if out is not None else make(total)
        if total > 0:
            if int(links.shape[0]) < total or (dist is not None and int(dist.numel()) < total):
                raise ValueError("%s: %d pairs, but `out` holds fewer entries" % (what, total))
            _check(call(links, dist, total, count), what)
            keys = (links[:total, 0].to(torch.int64) << 32) | links[:total, 1].to(torch.int64)
            order = torch.argsort(keys)
            links[:total] = links[:total][order]
            if dist is not None:
                dist[:total] = dist[:total][order]
    return links[:total], None if dist is None else dist[:total], count


def sketch_links(sketches, sizes, k, min_jaccard, capacity=None, with_dist=True, out=None, stream=None):
    """The pairs i < j of sketch rows [n, s] with sizes [n] that kmc_sketch_cluster links at
    min_jaccard (kmc_sketch_links): neither row empty and shared >= min_jaccard * denom.
    Returns (links int32 [., 4], dist float32 [.] or None, num_links int64 [1]): a row of
    links is (i, j, shared, denom), dist its Mash distance at k (with_dist=False: None,
    not computed), num_links the number of listed pairs whether they fit or not.
      capacity=N     asynchronous on the stream.  The tensors hold N entries, of which the
                     first min(num_links, N) are written, in no particular order;
                     capacity=0 is the count-only call (nothing but num_links is written).
      capacity=None  the convenience form, SYNCHRONOUS: a count-only call, a wait for the
                     stream, tensors of exactly num_links entries, a second call, and the
                     entries sorted by (i, j).
    `out` is the caller's own triple (links, dist or None, num_links); links and dist may be
    longer than capacity (nothing is written at or beyond it)."""
    with _on(stream):
        sketches = sketches.contiguous()
    n, s = int(sketches.shape[0]), int(sketches.shape[1])

    def call(links, dist, cap, count):
        return lib().kmc_sketch_links(_dptr(sketches), _dptr(sizes), n, s, k, float(min_jaccard), _dptr(links),
                                      _dptr(dist), cap, _dptr(count), _stream(stream))
    return _links(call, "kmc_sketch_links", sketches.device, capacity, with_dist, out, stream)


def sketch_links_rect(q, qs, r, rs, k, min_jaccard, capacity=None, with_dist=True, out=None, stream=None):
    """The pairs of a query row (q [m, s], sizes qs) and a reference row (r [n, s], sizes
    rs) that the rule of sketch_links accepts (kmc_sketch_links_rect): a row of links is
    (query, reference, shared, denom).  Forms, results and `out` as sketch_links; the
    capacity=None form is synchronous and sorts by (query, reference)."""
    q, r, m, n, s = _row_sets(q, r, stream)

    def call(links, dist, cap, count):
        return lib().kmc_sketch_links_rect(_dptr(q), _dptr(qs), m, _dptr(r), _dptr(rs), n, s, k, float(min_jaccard),
                                           _dptr(links), _dptr(dist), cap, _dptr(count), _stream(stream))
    return _links(call, "kmc_sketch_links_rect", q.device, capacity, with_dist, out, stream)


SCREEN_MAX_VALUES = 1 << 30


def sketch_screen_index_size(num_refs, sketch_size):
    return int(lib().kmc_sketch_screen_index_size(num_refs, sketch_size))


def sketch_screen_build(r, rs, index=None, stream=None):
    """The screen index (kmc_sketch_screen_build) of reference rows r [n, s] with sizes
    rs [n]: a uint8 device tensor of sketch_screen_index_size(n, s) bytes, or the
    caller's own `index` (a larger one is fine).  Every multiplicity starts at 0."""
    import torch
    with _on(stream):
        r = r.contiguous()
        n, s = int(r.shape[0]), int(r.shape[1])
        if index is None:
            index = torch.empty(sketch_screen_index_size(n, s), dtype=torch.uint8, device=r.device)
    rc = lib().kmc_sketch_screen_build(_dptr(r), _dptr(rs), n, s, *_ws(index), _stream(stream))
    _check(rc, "kmc_sketch_screen_build")
    return index


def sketch_screen_count(index, data, indices, k, flags=0, seed=SKETCH_DEFAULT_SEED, data_bytes=None, stream=None):
    """Adds the windows of the records (data, indices: as sketch_from_sequences) to the
    multiplicities of `index` (kmc_sketch_screen_count); calls accumulate."""
    n = int(indices.numel() - 1)
    if data_bytes is None:
        data_bytes = data.numel()
    rc = lib().kmc_sketch_screen_count(*_ws(index), _dptr(data), _dptr(indices), n, int(data_bytes), k, flags,
                                       int(seed) & _M64, _stream(stream))
    _check(rc, "kmc_sketch_screen_count")


def sketch_screen_results(index, r, rs, k, median=True, identity=True, out=None, stream=None):
    """What `index` holds of the rows r [n, s] with sizes rs [n]
    (kmc_sketch_screen_results): (shared int32 [n], median multiplicity int32 [n] or
    None, containment identity float32 [n] or None); `out`: the caller's own triple."""
    import torch
    with _on(stream):
        r = r.contiguous()
        n, s = int(r.shape[0]), int(r.shape[1])
        if out is not None:
            sh, med, ident = out
        else:
            sh = torch.empty(n, dtype=torch.int32, device=r.device)
            med = torch.empty(n, dtype=torch.int32, device=r.device) if median else None
            ident = torch.empty(n, dtype=torch.float32, device=r.device) if identity else None
    rc = lib().kmc_sketch_screen_results(*_ws(index), _dptr(r), _dptr(rs), n, s, k, _dptr(sh), _dptr(med),
                                         _dptr(ident), _stream(stream))
    _check(rc, "kmc_sketch_screen_results")
    return sh, med, ident


def sketch_screen_winners_workspace_size(index, num_refs):
    """Bytes of sketch_screen_winners' workspace for `index` (the tensor, or its size in
    bytes) and num_refs rows; 0 on bad arguments and for no row."""
    nbytes = index if isinstance(index, int) else index.numel() * index.element_size()
    return int(lib().kmc_sketch_screen_winners_workspace_size(nbytes, num_refs))


def sketch_screen_winners(index, r, rs, k, median=True, identity=True, shared_all=True, workspace=None, out=None,
                          stream=None):
    """The results with every found value credited to the best row that holds it only
    (kmc_sketch_screen_winners; Mash's screen -w): (won int32 [n], median multiplicity of
    the won values int32 [n] or None, identity of won / size float32 [n] or None,
    sketch_screen_results' shared int32 [n] or None); `out`: the caller's own four."""
    import torch
    with _on(stream):
        r = r.contiguous()
        n, s = int(r.shape[0]), int(r.shape[1])
        if out is not None:
            won, med, ident, sh = out
        else:
            won = torch.empty(n, dtype=torch.int32, device=r.device)
            med = torch.empty(n, dtype=torch.int32, device=r.device) if median else None
            ident = torch.empty(n, dtype=torch.float32, device=r.device) if identity else None
            sh = torch.empty(n, dtype=torch.int32, device=r.device) if shared_all else None
    rc = lib().kmc_sketch_screen_winners(*_ws(index), _dptr(r), _dptr(rs), n, s, k, _dptr(won), _dptr(med),
                                         _dptr(ident), _dptr(sh), *_ws(workspace), _stream(stream))
    _check(rc, "kmc_sketch_screen_winners")
    return won, med, ident, sh


SKETCH_ACCUM_MIN_LOG2_SLOTS = 4
SKETCH_ACCUM_MAX_LOG2_SLOTS = 30


def sketch_accum_device_bytes(sketch_size, log2_slots=0):
    """Device bytes a SketchAccum of these two numbers holds (0 on bad arguments)."""
    return int(lib().kmc_sketch_accum_device_bytes(int(sketch_size), int(log2_slots)))


class SketchAccum:
    """kmc_sketch_accum_*: the bottom-s sketch of the k-mers seen at least min_count
    times over any number of batches (a read set of any size).  add() takes a batch
    of records (data, indices: as sketch_from_sequences); finish(min_count) returns
    (row int64 [s]: uint64 hashes ascending, then all-ones fill; size int32 [1];
    stats int64 [4]: complete, limit, tracked, qualifying, or None) and leaves the
    accumulator as it is; spectrum(num_bins) gives the abundance spectrum of what was
    added (kmc_spectrum_from_accum), and leaves it as it is too; match(data, indices)
    says per record how many of its k-mers are among what was added
    (kmc_match_from_accum), and leaves it as it is too; reset() empties it.  `log2_slots`: the table's size, 0 for
    the default (kmc.h).  The handle belongs to the library it was created in.

        with kmc.SketchAccum(1000, 21) as acc:
            with kmc.FastqReader(path, 1 << 28, copy=False) as rd:
                for data, indices in rd:
                    acc.add(data, indices)
            row, size, stats = acc.finish(min_count=2)"""

    def __init__(self, sketch_size, k, flags=0, seed=SKETCH_DEFAULT_SEED, log2_slots=0):
        self._h = _P()
        self._lib = lib()
        self.sketch_size = int(sketch_size)
        _check(self._lib.kmc_sketch_accum_create(self.sketch_size, int(k), int(flags), int(seed) & _M64,
                                                 int(log2_slots), ctypes.byref(self._h)), "kmc_sketch_accum_create")

    def _handle(self):
        if not self._h:
            raise ValueError("the accumulator is closed")
        return self._h

    def add(self, data, indices, data_bytes=None, stream=None):
        h = self._handle()
        n = int(indices.numel() - 1)
        if data_bytes is None:
            data_bytes = data.numel()
        _check(self._lib.kmc_sketch_accum_add(h, _dptr(data), _dptr(indices), n, int(data_bytes),
                                              _stream(stream)), "kmc_sketch_accum_add")

    def finish(self, min_count=1, stats=True, out=None, stream=None):
        """`stats`: True for a new tensor, or the caller's own int64 tensor [4]; `out`:
        the caller's own (row, size)."""
        import torch
        h = self._handle()
        with _on(stream):
            dv = torch.device("cuda", torch.cuda.current_device())
            row, size = out if out is not None else (torch.empty(self.sketch_size, dtype=torch.int64, device=dv),
                                                     torch.empty(1, dtype=torch.int32, device=dv))
            if isinstance(stats, torch.Tensor):
                st = stats
            else:
                st = torch.empty(4, dtype=torch.int64, device=dv) if stats else None
        _check(self._lib.kmc_sketch_accum_finish(h, int(min_count), _dptr(row), _dptr(size), _dptr(st),
                                                 _stream(stream)), "kmc_sketch_accum_finish")
        return row, size, st

    def spectrum(self, num_bins, stats=True, out=None, stream=None):
        """kmc_spectrum_from_accum: (hist int64 [num_bins]: uint64 numbers of tracked
        k-mers seen c times, the last bin saturating; stats int64 [4]: exact, limit,
        entries, windows, or None) of everything added so far, for the k-mers below the
        limit finish() reports.  It leaves the accumulator as it is.  `stats`: True for
        a new tensor, or the caller's own int64 tensor [4]; `out`: the caller's own hist."""
        import torch
        h = self._handle()
        with _on(stream):
            dv = torch.device("cuda", torch.cuda.current_device())
            hist = out if out is not None else torch.empty(max(int(num_bins), 0), dtype=torch.int64, device=dv)
            if isinstance(stats, torch.Tensor):
                st = stats
            else:
                st = torch.empty(4, dtype=torch.int64, device=dv) if stats else None
        _check(self._lib.kmc_spectrum_from_accum(h, int(num_bins), _dptr(hist), _dptr(st), _stream(stream)),
               "kmc_spectrum_from_accum")
        return hist, st

    def match(self, data, indices, min_count=1, windows=True, sampled=True, stats=True, data_bytes=None, out=None,
              stream=None):
        """kmc_match_from_accum: per record of (data, indices: as add) how many of its
        windows are valid, how many of those are sampled (all of them when the table
        held everything, else those with a hash below the limit finish() reports) and
        how many of those are in the set with count >= min_count.  Returns (windows,
        sampled, hits: int32 [n] holding uint32 numbers; stats int64 [4]: exact, limit,
        sum of sampled, sum of hits), with None for what was not asked for.  It leaves
        the accumulator as it is.  `windows`, `sampled`: True for a new tensor, False or
        None for none, or the caller's own int32 tensor [n]; `stats`: the same with an
        int64 tensor [4]; `out`: the caller's own hits."""
        import torch
        h = self._handle()
        n = int(indices.numel() - 1)
        if data_bytes is None:
            data_bytes = data.numel()
        with _on(stream):
            dv = torch.device("cuda", torch.cuda.current_device())

            def take(want, count, dtype):
                if isinstance(want, torch.Tensor):
                    return want
                return torch.empty(max(count, 0), dtype=dtype, device=dv) if want else None
            win, smp = take(windows, n, torch.int32), take(sampled, n, torch.int32)
            hit = out if out is not None else take(True, n, torch.int32)
            st = take(stats, 4, torch.int64)
            # (no record: an empty tensor has no address, and the library refuses a null hits; nothing is written there)
            hits_at = hit if hit.numel() else torch.empty(1, dtype=torch.int32, device=dv)
        _check(self._lib.kmc_match_from_accum(h, _dptr(data), _dptr(indices), n, int(data_bytes), int(min_count),
                                              _dptr(win), _dptr(smp), _dptr(hits_at), _dptr(st), _stream(stream)),
               "kmc_match_from_accum")
        return win, smp, hit, st

    def label(self, data, indices, source, data_bytes=None, stream=None):
        """kmc_label_accum: the k-mers of the records (data, indices: as add) that
        are in the set get bit `source` (0 .. 31) in their label.  All adds come first:
        an add of records or a reset drops the labels.  It leaves the set as it is."""
        h = self._handle()
        n = int(indices.numel() - 1)
        if data_bytes is None:
            data_bytes = data.numel()
        _check(self._lib.kmc_label_accum(h, _dptr(data), _dptr(indices), n, int(data_bytes), int(source),
                                                _stream(stream)), "kmc_label_accum")

    def classify(self, data, indices, num_sources, min_count=1, windows=True, sampled=True, scores=False, stats=True,
                 data_bytes=None, workspace=None, out=None, stream=None):
        """kmc_classify_from_accum: match() with the votes of the labelled sources.
        Returns (windows, sampled, hits, best, best_hits, next_hits: int32 [n] holding
        uint32 numbers; scores: int32 [n, num_sources] or None; stats int64 [4]).  best is
        the smallest source with the most hit windows, CLASSIFY_NONE (-1 as int32) when
        no source has one; best_hits its score and next_hits the runner-up's.  `windows`,
        `sampled`, `scores`, `stats`: as match's; `out`: the caller's own (hits, best,
        best_hits, next_hits); `workspace`: a tensor of classify_workspace_size() bytes,
        None for the library's own."""
        import torch
        h = self._handle()
        n = int(indices.numel() - 1)
        ns = int(num_sources)
        if data_bytes is None:
            data_bytes = data.numel()
        with _on(stream):
            dv = torch.device("cuda", torch.cuda.current_device())

            def take(want, shape, dtype):
                if isinstance(want, torch.Tensor):
                    return want
                return torch.empty(shape, dtype=dtype, device=dv) if want else None
            n0 = max(n, 0)
            win, smp = take(windows, n0, torch.int32), take(sampled, n0, torch.int32)
            hit, best, bh, nh = out if out is not None else [take(True, n0, torch.int32) for _ in range(4)]
            sc = take(scores, (n0, max(ns, 0)), torch.int32)
            st = take(stats, 4, torch.int64)
            # (no record: an empty tensor has no address, and the library refuses null outputs; nothing is written there)
            spare = torch.empty(1, dtype=torch.int32, device=dv) if n0 == 0 else None
            at = [t if t.numel() else spare for t in (hit, best, bh, nh)]
        ws, ws_bytes = _ws(workspace)
        _check(self._lib.kmc_classify_from_accum(h, _dptr(data), _dptr(indices), n, int(data_bytes), ns, int(min_count),
                                                 _dptr(win), _dptr(smp), _dptr(at[0]), _dptr(at[1]), _dptr(at[2]),
                                                 _dptr(at[3]), _dptr(sc) if sc is not None and sc.numel() else None,
                                                 _dptr(st), ws, ws_bytes, _stream(stream)), "kmc_classify_from_accum")
        return win, smp, hit, best, bh, nh, sc, st

    def reset(self, stream=None):
        _check(self._lib.kmc_sketch_accum_reset(self._handle(), _stream(stream)), "kmc_sketch_accum_reset")

    def close(self):
        if self._h:
            self._lib.kmc_sketch_accum_free(self._h)
            self._h = _P()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()


SPECTRUM_MAX_BINS = 8192
SpectrumResult = collections.namedtuple("SpectrumResult", [f[0] for f in SpectrumSummary._fields_])


def select_records_workspace_size(num_recs, src_bytes):
    return int(lib().kmc_select_records_workspace_size(int(num_recs), int(src_bytes)))


def select_records(src, offsets, keep, invert=False, capacity=None, offsets_out=True, src_bytes=None, workspace=None,
                   out=None, stream=None):
    """kmc_select_records: the records src[offsets[r]:offsets[r+1]] (src uint8, offsets
    int64 [n+1], on the device) with (keep[r] != 0) != invert, concatenated in input
    order.  keep: int32 or uint32 [n]; any non-zero value selects, so the hits of
    SketchAccum.match serve.  Returns (dst uint8 [capacity], dst_offsets int64 [n+1] or
    None, counts int64 [2]: the selected records and their bytes), all on the device
    and nothing read back: dst[:counts[1]] and dst_offsets[:counts[0] + 1] are the
    result, a record buffer again.  capacity: None for src's size, which always
    suffices; 0 counts only.  offsets_out: True for a new tensor, False for none, or
    the caller's own; out: the caller's own (dst, counts)."""
    import torch
    n = int(offsets.numel() - 1)
    if src_bytes is None:
        src_bytes = src.numel()
    with _on(stream):
        dv = torch.device("cuda", torch.cuda.current_device())
        if out is not None:
            dst, counts = out
            cap = dst.numel() if capacity is None else int(capacity)
        else:
            cap = int(src_bytes) if capacity is None else int(capacity)
            dst = torch.empty(cap, dtype=torch.uint8, device=dv)
            counts = torch.empty(2, dtype=torch.int64, device=dv)
        if isinstance(offsets_out, torch.Tensor):
            doff = offsets_out
        else:
            doff = torch.empty(n + 1, dtype=torch.int64, device=dv) if offsets_out else None
        # (no record: an empty tensor has no address, and the library refuses a null keep; nothing is read there)
        keep_at = keep if keep.numel() else torch.empty(1, dtype=torch.int32, device=dv)
    ws, ws_bytes = _ws(workspace)
    _check(lib().kmc_select_records(_dptr(src) if src.numel() else None, _dptr(offsets), n, int(src_bytes),
                                    _dptr(keep_at), 1 if invert else 0, _dptr(dst) if cap else None, cap, _dptr(doff),
                                    _dptr(counts), ws, ws_bytes, _stream(stream)), "kmc_select_records")
    return dst, doff, counts


def match_select(sampled, hits, min_hits=1, min_fraction=0.0, count=True, out=None, stream=None):
    """kmc_match_select: keep[r] = hits[r] >= min_hits and hits[r] >= min_fraction *
    sampled[r] (in double), the rule of `kmc --recruit`, as int32 [n] of ones and zeros
    on the device.  sampled may be None when min_fraction is 0.  Returns (keep,
    num_kept int64 [1] or None)."""
    import torch
    n = int(hits.numel())
    with _on(stream):
        dv = torch.device("cuda", torch.cuda.current_device())
        keep = out if out is not None else torch.empty(n, dtype=torch.int32, device=dv)
        if isinstance(count, torch.Tensor):
            kept = count
        else:
            kept = torch.empty(1, dtype=torch.int64, device=dv) if count else None
    _check(lib().kmc_match_select(_dptr(sampled) if n else None, _dptr(hits) if n else None, n, int(min_hits),
                                  float(min_fraction), _dptr(keep) if n else None, _dptr(kept), _stream(stream)),
           "kmc_match_select")
    return keep, kept


CLASSIFY_MAX_SOURCES = 32
CLASSIFY_NONE = 0xFFFFFFFF


def classify_workspace_size(num_seqs, data_bytes, num_sources, device=0):
    return int(lib().kmc_classify_workspace_size(int(num_seqs), int(data_bytes), int(num_sources), int(device)))


def classify_select(listed, best, best_hits, next_hits, source, min_margin=1, count=True, out=None, stream=None):
    """kmc_classify_select: keep[r] = listed[r] != 0 and best[r] == source and best_hits[r]
    - next_hits[r] >= min_margin, the rule of `kmc --recruit --classify`, as int32 [n] of
    ones and zeros on the device.  listed (match_select's keep) may be None: every record;
    `out` may be listed itself.  Returns (keep, num_kept int64 [1] or None)."""
    import torch
    n = int(best.numel())
    with _on(stream):
        dv = torch.device("cuda", torch.cuda.current_device())
        keep = out if out is not None else torch.empty(n, dtype=torch.int32, device=dv)
        if isinstance(count, torch.Tensor):
            kept = count
        else:
            kept = torch.empty(1, dtype=torch.int64, device=dv) if count else None
    _check(lib().kmc_classify_select(_dptr(listed) if n else None, _dptr(best) if n else None,
                                     _dptr(best_hits) if n else None, _dptr(next_hits) if n else None, n, int(source),
                                     int(min_margin), _dptr(keep) if n else None, _dptr(kept), _stream(stream)),
           "kmc_classify_select")
    return keep, kept


def spectrum_summarize(hist, limit):
    """kmc_spectrum_summarize of a spectrum (SketchAccum.spectrum's hist, a tensor or a
    host array of uint64 bit patterns) and its limit (stats[1]): a namedtuple of the
    fields of kmc_spectrum_summary (kmc.h).  Host only."""
    if hasattr(hist, "cpu"):
        hist = hist.cpu().numpy()
    h = np.ascontiguousarray(hist)
    h = h.view(np.uint64) if h.dtype == np.int64 else h.astype(np.uint64)
    out = SpectrumSummary()
    _check(lib().kmc_spectrum_summarize(h.ctypes.data_as(_P), int(h.size), int(limit) & _M64, ctypes.byref(out)),
           "kmc_spectrum_summarize")
    return SpectrumResult(*[getattr(out, f[0]) for f in SpectrumSummary._fields_])


def min_kmeres2(sums, mins, num_seqs, current_seq, indexes, stream=None):
    """Drop-in of one reference minKmeres2 launch (k = 3, int32 indexes)."""
    rc = lib().minKmeres2_hip(_dptr(sums), _dptr(mins), num_seqs, current_seq, _dptr(indexes), _stream(stream))
    _check(rc, "minKmeres2_hip")


def trace_events(before=None, after=None):
    """Record torch.cuda.Event `before`/`after` around the next dense count kernels."""
    b = ctypes.c_void_p(before._as_parameter_.value) if before is not None else None
    a = ctypes.c_void_p(after._as_parameter_.value) if after is not None else None
    _check(lib().kmc_trace_set_events(b, a), "kmc_trace_set_events")


def set_reserved_cus(n):
    """Leave n CUs out of the dense (k <= 8) grid, for a concurrent kernel (kmc.h)."""
    _check(lib().kmc_set_reserved_cus(int(n)), "kmc_set_reserved_cus")


def synth_fill(data, num_records, record_len, seed, first_base=0, stream=None):
    rc = lib().kmc_synth_fill(_dptr(data), num_records, record_len, seed, first_base, _stream(stream))
    _check(rc, "kmc_synth_fill")


def synth_fill_range(data, lo, hi, record_len, seed, stream=None):
    """Global bytes [lo, hi) of the synthetic record stream into data[0 .. hi-lo)."""
    rc = lib().kmc_synth_fill_range(_dptr(data), lo, hi, record_len, seed, _stream(stream))
    _check(rc, "kmc_synth_fill_range")


def synth_indices(num_records, record_len):
    out = np.zeros(num_records + 1, dtype=np.int64)
    lib().kmc_synth_indices(out.ctypes.data_as(_P), num_records, record_len)
    return out


# ---------------------------------------------------------------------------
# sharding (host planning; device work in kmc_dist.py / kmc_count_multi)
# ---------------------------------------------------------------------------
class Shard(ctypes.Structure):
    _fields_ = [("win_lo", _U64), ("win_hi", _U64), ("read_lo", _U64), ("read_hi", _U64)]


def plan_shards(indices, k, nshards, align=4096):
    """Byte-balanced shards of [indices[0], indices[-1]): list of (win_lo, win_hi, read_lo, read_hi)."""
    idx = np.ascontiguousarray(indices, dtype=np.int64)
    out = (Shard * nshards)()
    _check(lib().kmc_plan_shards(idx.ctypes.data_as(_P), idx.size - 1, k, nshards, align, out), "kmc_plan_shards")
    return [(s.win_lo, s.win_hi, s.read_lo, s.read_hi) for s in out]


def count_multi(data, indices, k, ndev=1, devices=None, invalid=False):
    """Single-process multi-GPU count of a host buffer (kmc_count_multi: shards + RCCL all-reduce)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    idx = np.ascontiguousarray(indices, dtype=np.int64)
    n = idx.size - 1
    out = np.zeros((1 << (2 * k), n), dtype=np.int32)
    inv = np.zeros(n, dtype=np.int32) if invalid else None
    devs = None
    if devices is not None:
        devs = (ctypes.c_int * ndev)(*devices)
    rc = lib().kmc_count_multi(data.ctypes.data_as(_P), idx.ctypes.data_as(_P), n, data.size, k, ndev, devs,
                               out.ctypes.data_as(_P), inv.ctypes.data_as(_P) if inv is not None else None)
    _check(rc, "kmc_count_multi")
    return out, inv


# ---------------------------------------------------------------------------
# host: FASTA loader
# ---------------------------------------------------------------------------
def load_fasta(path, dialect=DIALECT_BLANK, max_seqs=MAX_SEQS_REFERENCE):
    """Returns (data uint8, indices int64 [n+1], reference_num_indexes)."""
    L = lib()
    h = _P()
    _check(L.kmc_fasta_load(os.fsencode(path), dialect, max_seqs, ctypes.byref(h)), "kmc_fasta_load")
    try:
        n = L.kmc_fasta_num_seqs(h)
        nbytes = L.kmc_fasta_data_bytes(h)
        idx = np.ctypeslib.as_array(ctypes.cast(L.kmc_fasta_indices(h), ctypes.POINTER(_I64)), (n + 1,)).copy()
        if nbytes:
            data = np.ctypeslib.as_array(ctypes.cast(L.kmc_fasta_data(h), ctypes.POINTER(ctypes.c_uint8)),
                                         (nbytes,)).copy()
        else:
            data = np.zeros(0, dtype=np.uint8)
        ref_n = L.kmc_fasta_reference_num_indexes(h)
    finally:
        L.kmc_fasta_free(h)
    return data, idx, int(ref_n)


def parse_fasta_device(raw, dialect=DIALECT_BLANK, stream=None):
    """GPU FASTA parse (kmc_fasta_parse_device) of raw file bytes in a uint8 device
    tensor; returns (data uint8 tensor, indices int64 tensor [n+1]) on its device."""
    import torch
    n = int(raw.numel())
    with _on(stream):
        if n % 16 or raw.data_ptr() % 16:  # the kernel reads whole 16-byte pieces of raw
            pad = torch.zeros(n + 16 - n % 16, dtype=torch.uint8, device=raw.device)
            pad[:n] = raw
            raw = pad
        data = torch.empty(n + 16, dtype=torch.uint8, device=raw.device)
    cap = 1024
    while True:
        with _on(stream):
            idx = torch.empty(cap, dtype=torch.int64, device=raw.device)
        ns, nb = _U64(0), _U64(0)
        rc = lib().kmc_fasta_parse_device(_dptr(raw) if n else None, n, dialect, _dptr(data), n + 16, _dptr(idx),
                                          cap, ctypes.byref(ns), ctypes.byref(nb), _stream(stream))
        if rc == KMC_ERR_CAPACITY and ns.value + 1 > cap:
            cap = int(ns.value) + 1
            continue
        _check(rc, "kmc_fasta_parse_device")
        return data[:nb.value], idx[:ns.value + 1]


def load_fasta_device(path, dialect=DIALECT_BLANK, max_seqs=MAX_SEQS_REFERENCE, stream=None):
    """kmc_fasta_load_device: (data uint8 tensor, indices int64 tensor [n+1]) on the
    current device (copies of the library's buffers, which are freed here)."""
    import torch
    L = lib()
    d, ix = _P(), _P()
    nb, ns = _U64(0), _U64(0)
    _check(L.kmc_fasta_load_device(os.fsencode(path), dialect, max_seqs, ctypes.byref(d), ctypes.byref(nb),
                                   ctypes.byref(ix), ctypes.byref(ns), _stream(stream)), "kmc_fasta_load_device")
    dev = torch.device("cuda", torch.cuda.current_device())
    data = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    idx = torch.empty(ns.value + 1, dtype=torch.int64, device=dev)
    hip = _hip()
    if nb.value:
        _check(hip.hipMemcpy(_P(data.data_ptr()), d, nb.value, 3), "hipMemcpy")
    _check(hip.hipMemcpy(_P(idx.data_ptr()), ix, (ns.value + 1) * 8, 3), "hipMemcpy")
    hip.hipFree(d)
    hip.hipFree(ix)
    return data, idx


def _copy_out(d, nbytes, ix, nseqs, free):
    """New torch tensors (data uint8 [nbytes], indices int64 [nseqs + 1]) on the current
    device holding the library's buffers d and ix, which are freed when `free`."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    data = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idx = torch.empty(nseqs + 1, dtype=torch.int64, device=dev)
    hip = _hip()
    if nbytes:
        _check(hip.hipMemcpy(_P(data.data_ptr()), d, nbytes, 3), "hipMemcpy")
    _check(hip.hipMemcpy(_P(idx.data_ptr()), ix, (nseqs + 1) * 8, 3), "hipMemcpy")
    if free:
        hip.hipFree(d)
        hip.hipFree(ix)
    return data, idx


# ---------------------------------------------------------------------------
# FASTQ (strict four-line; include/kmc.h)
# ---------------------------------------------------------------------------
def parse_fastq_device(raw, final=True, stream=None, raw_indices=False):
    """GPU FASTQ parse (kmc_fastq_parse_device) of raw bytes in a uint8 device tensor:
    (data uint8 tensor, indices int64 tensor [n+1], consumed) for the complete
    records of raw; without `final` the bytes from `consumed` on belong to a record
    that is not complete yet.  KmcError.record tells where malformed input is.
    With raw_indices (kmc_fastq_parse_device_ex) a fourth value follows: the int64
    tensor [n+1] of the records' raw offsets, record r's full text being
    raw[raw_indices[r]:raw_indices[r+1]]."""
    import torch
    n = int(raw.numel())
    with _on(stream):
        if n % 16 or raw.data_ptr() % 16:  # the kernel reads whole 16-byte pieces of raw
            pad = torch.zeros(n + 16 - n % 16, dtype=torch.uint8, device=raw.device)
            pad[:n] = raw
            raw = pad
        cap_data = n // 2 + 1
        data = torch.empty(cap_data + 16, dtype=torch.uint8, device=raw.device)
    cap = 1024
    while True:
        with _on(stream):
            idx = torch.empty(cap, dtype=torch.int64, device=raw.device)
            ridx = torch.empty(cap, dtype=torch.int64, device=raw.device) if raw_indices else None
        ns, nb, used = _U64(0), _U64(0), _U64(0)
        if raw_indices:
            rc = lib().kmc_fastq_parse_device_ex(_dptr(raw) if n else None, n, 1 if final else 0, _dptr(data), cap_data,
                                                 _dptr(idx), cap, ctypes.byref(ns), ctypes.byref(nb), ctypes.byref(used),
                                                 _dptr(ridx), _stream(stream))
        else:
            rc = lib().kmc_fastq_parse_device(_dptr(raw) if n else None, n, 1 if final else 0, _dptr(data), cap_data,
                                              _dptr(idx), cap, ctypes.byref(ns), ctypes.byref(nb), ctypes.byref(used),
                                              _stream(stream))
        if rc == KMC_ERR_CAPACITY and ns.value + 1 > cap:
            cap = int(ns.value) + 1
            continue
        _check(rc, "kmc_fastq_parse_device", ns.value)
        if raw_indices:
            return data[:nb.value], idx[:ns.value + 1], int(used.value), ridx[:ns.value + 1]
        return data[:nb.value], idx[:ns.value + 1], int(used.value)


def load_fastq_device(path, max_seqs=0, stream=None):
    """kmc_fastq_load_device: (data uint8 tensor, indices int64 tensor [n+1]) on the
    current device (copies of the library's buffers, which are freed here);
    max_seqs > 0 keeps the first max_seqs records."""
    L = lib()
    d, ix = _P(), _P()
    nb, ns = _U64(0), _U64(0)
    _check(L.kmc_fastq_load_device(os.fsencode(path), max_seqs, ctypes.byref(d), ctypes.byref(nb), ctypes.byref(ix),
                                   ctypes.byref(ns), _stream(stream)), "kmc_fastq_load_device", ns.value)
    return _copy_out(d, nb.value, ix, ns.value, True)


class FastqReader:
    """kmc_fastq_open / _next / _close: a FASTQ file of any size (or a pipe) as batches
    of about batch_bytes raw bytes (0: 256 MiB).  next_batch() returns (data,
    indices) or None after the last batch; iterating yields the batches.  By default
    a batch is a pair of new tensors (copies); with copy=False it is a pair of views
    of the reader's own buffers, valid until the next call, whose writes are ordered
    on `stream` behind whatever the caller enqueued there.  With keep_raw=True
    (KMC_FASTQ_KEEP_RAW) raw() returns the last batch's raw text and the records'
    raw offsets, what select_records cuts the reads themselves from.

        with kmc.FastqReader(path, 1 << 28) as rd:
            for data, indices in rd:
                kmc.sketch_screen_count(index, data, indices, k)"""

    def __init__(self, path, batch_bytes=0, stream=None, copy=True, keep_raw=False):
        self._h = _P()
        self._stream = stream
        self._copy = copy
        self._views = None
        self._seqs = 0
        if keep_raw:
            _check(lib().kmc_fastq_open_ex(os.fsencode(path), int(batch_bytes), KMC_FASTQ_KEEP_RAW, ctypes.byref(self._h)),
                   "kmc_fastq_open_ex")
        else:
            _check(lib().kmc_fastq_open(os.fsencode(path), int(batch_bytes), ctypes.byref(self._h)), "kmc_fastq_open")

    def raw(self):
        """kmc_fastq_raw: (raw uint8 tensor [raw_bytes], raw_indices int64 tensor [n+1]) of
        the last batch, or None after the last batch: views of the reader's own buffers,
        valid until the next call on the reader (clone them to keep them)."""
        if not self._h:
            raise ValueError("the reader is closed")
        d, ix, nb = _P(), _P(), _U64(0)
        _check(lib().kmc_fastq_raw(self._h, ctypes.byref(d), ctypes.byref(nb), ctypes.byref(ix)), "kmc_fastq_raw")
        if not d.value:
            return None
        return (_DeviceView(d.value, nb.value, "|u1").tensor(), _DeviceView(ix.value, self._seqs + 1, "<i8").tensor())

    def next_batch(self):
        if not self._h:
            raise ValueError("the reader is closed")
        d, ix = _P(), _P()
        nb, ns = _U64(0), _U64(0)
        rc = lib().kmc_fastq_next(self._h, ctypes.byref(d), ctypes.byref(nb), ctypes.byref(ix), ctypes.byref(ns),
                                  _stream(self._stream))
        _check(rc, "kmc_fastq_next", ns.value)
        self._seqs = int(ns.value)
        if not d.value:
            return None
        if self._copy:
            return _copy_out(d, nb.value, ix, ns.value, False)
        self._views = (_DeviceView(d.value, nb.value, "|u1").tensor(), _DeviceView(ix.value, ns.value + 1, "<i8").tensor())
        return self._views

    def close(self):
        if self._h:
            lib().kmc_fastq_close(self._h)
            self._h = _P()

    def __iter__(self):
        return self

    def __next__(self):
        b = self.next_batch()
        if b is None:
            raise StopIteration
        return b

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()


class _DeviceView:
    """A device buffer the library owns as a torch tensor, without a copy
    (__cuda_array_interface__); count elements of numpy typestr `typestr`."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2}
        self._count = int(count)
        self._typestr = typestr

    def tensor(self):
        import torch
        if self._count == 0:
            return torch.empty(0, dtype=torch.uint8 if self._typestr == "|u1" else torch.int64,
                               device=torch.device("cuda", torch.cuda.current_device()))
        return torch.as_tensor(self, device=torch.device("cuda", torch.cuda.current_device()))


_hip_lib = None


def _hip():
    global _hip_lib
    if _hip_lib is None:
        _hip_lib = ctypes.CDLL("libamdhip64.so.7")  # by SONAME: the runtime libkmc.so is bound to
        _hip_lib.hipMemcpy.argtypes = [_P, _P, ctypes.c_size_t, ctypes.c_int]
        _hip_lib.hipFree.argtypes = [_P]
    return _hip_lib


# ---------------------------------------------------------------------------
# host reference of the synthetic generator (tests compare the kernel to it)
# ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def splitmix64_np(seed, n):
    """Outputs n of splitmix64 (numpy uint64 array in, array out)."""
    n = np.asarray(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (n + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def synth_host_range(lo, hi, record_len, seed):
    """Same bytes as kmc_synth_fill_range, on the host (small sizes)."""
    p = np.arange(lo, hi, dtype=np.uint64)
    rb = np.uint64(record_len + 1)
    r, off = p // rb, p % rb
    g = r * np.uint64(record_len) + off
    words = splitmix64_np(seed, g >> np.uint64(5))
    codes = ((words >> (np.uint64(2) * (g & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)
    out = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    out[off == np.uint64(record_len)] = 0
    return out


def synth_host(num_records, record_len, seed, first_base=0):
    """Same bytes as kmc_synth_fill, on the host (small sizes)."""
    g = np.arange(num_records * record_len, dtype=np.uint64) + np.uint64(first_base)
    words = splitmix64_np(seed, g >> np.uint64(5))
    codes = ((words >> (np.uint64(2) * (g & np.uint64(31)))) & np.uint64(3)).astype(np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[codes].reshape(num_records, record_len)
    out = np.zeros((num_records, record_len + 1), dtype=np.uint8)
    out[:, :record_len] = bases
    return out.reshape(-1)

"""The error contract of the six softmax-attention entry points without a GPU: which check refuses a bad call, in which order,
and with which words.  Every call below is refused with SRF_EINVAL before any launch (the pointers are dummies that no check
dereferences), and EXPECTED holds the message of each, recorded from the library as it was BEFORE the six entries came to share
one host path per direction: the order of the checks and every string are part of the interface (callers match on them).
(A head dimension off the MFMA grid, such as d = 24, is no refusal in any kernel mode -- the VALU form serves it -- so it has no
case here; tests/test_gpu_attention*.py run it.)"""
import ctypes as C

import pytest

P = C.c_void_p(0x1000)
POINTERS = {"srf_mha_attention": ("q", "k", "v", "o"),
            "srf_mha_attention_lse": ("q", "k", "v", "o", "lse"),
            "srf_mha_attention_bwd": ("q", "k", "v", "o", "lse", "go", "gq", "gk", "gv", "workspace")}
ENTRIES = tuple(POINTERS) + tuple(e + "_ragged" for e in POINTERS)
VALID = dict(Bt=3, H=2, d=16, Lq=9, Lk=7)
BAD_Q = ((C.c_int * 3)(9, 0, 3), None)          # example 1 has no query

# case -> (the pointer passed as NULL, the sizes that differ from VALID, (q_lengths, k_lengths) of the ragged entries)
CASES = {
    "null_q": ("q", {}, None),
    "null_lse": ("lse", {}, None),
    "null_workspace": ("workspace", {}, None),
    "H_0": (None, dict(H=0), None),
    "Bt_0": (None, dict(Bt=0), None),
    "Bt_65536": (None, dict(Bt=65536), None),
    "example_2e31": (None, dict(H=1024, d=1024, Lq=2048), None),          # H d Lq = 2^31
    "d_1025": (None, dict(d=1025), None),                                 # no MFMA form, and past the VALU form's 1024
    "bad_length": (None, {}, BAD_Q),                                      # ... after otherwise valid arguments
    "bad_length_and_null_q": ("q", {}, BAD_Q),                            # the uniform checks come first
    "bad_length_and_Bt_65536": (None, dict(Bt=65536), BAD_Q),
    "bad_length_and_d_1025": (None, dict(d=1025), BAD_Q),                 # forward: the tables, then the dispatch; backward: d first
}


def applies(entry, case):
    null, _, lengths = CASES[case]
    base = entry[:-len("_ragged")] if entry.endswith("_ragged") else entry
    return (null is None or null in POINTERS[base]) and (lengths is None or entry.endswith("_ragged"))


def call(lib, entry, case):
    """-> (return code, srf_last_error()) of `entry` called with VALID arguments but for what `case` changes"""
    null, sizes, lengths = CASES[case]
    ragged = entry.endswith("_ragged")
    s = dict(VALID, **sizes)
    args = [None if n == null else P for n in POINTERS[entry[:-len("_ragged")] if ragged else entry]]
    args += [s["Bt"], s["H"], s["d"], s["Lq"], s["Lk"]]
    if ragged:
        args += list(lengths or (None, None))
    rc = getattr(lib, entry)(*args, C.c_float(0.25), None)
    return rc, lib.srf_last_error().decode()


EXPECTED = {
    ("srf_mha_attention", "null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention", "H_0"):
        "srf_mha_attention: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention", "Bt_0"):
        "srf_mha_attention: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention", "Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention", "example_2e31"):
        "srf_mha_attention: one example exceeds 2^31 elements",
    ("srf_mha_attention", "d_1025"):
        "srf_mha_attention: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_lse", "null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention_lse", "null_lse"):
        "srf_mha_attention_lse: lse is null",
    ("srf_mha_attention_lse", "H_0"):
        "srf_mha_attention_lse: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_lse", "Bt_0"):
        "srf_mha_attention: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_lse", "Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_lse", "example_2e31"):
        "srf_mha_attention: one example exceeds 2^31 elements",
    ("srf_mha_attention_lse", "d_1025"):
        "srf_mha_attention: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_bwd", "null_q"):
        "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)",
    ("srf_mha_attention_bwd", "null_lse"):
        "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)",
    ("srf_mha_attention_bwd", "null_workspace"):
        "srf_mha_attention_bwd: workspace is null (srf_mha_attention_bwd_workspace_bytes)",
    ("srf_mha_attention_bwd", "H_0"):
        "srf_mha_attention_bwd: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_bwd", "Bt_0"):
        "srf_mha_attention_bwd: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_bwd", "Bt_65536"):
        "srf_mha_attention_bwd: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_bwd", "example_2e31"):
        "srf_mha_attention_bwd: one example exceeds 2^31 elements",
    ("srf_mha_attention_bwd", "d_1025"):
        "srf_mha_attention_bwd: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_ragged", "null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention_ragged", "H_0"):
        "srf_mha_attention_ragged: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_ragged", "Bt_0"):
        "srf_mha_attention: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_ragged", "Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_ragged", "example_2e31"):
        "srf_mha_attention: one example exceeds 2^31 elements",
    ("srf_mha_attention_ragged", "d_1025"):
        "srf_mha_attention: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_ragged", "bad_length"):
        "srf_mha_attention_ragged: example 1 has q_lengths[b] = 0 (allowed: 1..Lq = 9)",
    ("srf_mha_attention_ragged", "bad_length_and_null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention_ragged", "bad_length_and_Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_ragged", "bad_length_and_d_1025"):
        "srf_mha_attention_ragged: example 1 has q_lengths[b] = 0 (allowed: 1..Lq = 9)",
    ("srf_mha_attention_lse_ragged", "null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention_lse_ragged", "null_lse"):
        "srf_mha_attention_lse_ragged: lse is null",
    ("srf_mha_attention_lse_ragged", "H_0"):
        "srf_mha_attention_lse_ragged: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_lse_ragged", "Bt_0"):
        "srf_mha_attention: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_lse_ragged", "Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_lse_ragged", "example_2e31"):
        "srf_mha_attention: one example exceeds 2^31 elements",
    ("srf_mha_attention_lse_ragged", "d_1025"):
        "srf_mha_attention: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_lse_ragged", "bad_length"):
        "srf_mha_attention_lse_ragged: example 1 has q_lengths[b] = 0 (allowed: 1..Lq = 9)",
    ("srf_mha_attention_lse_ragged", "bad_length_and_null_q"):
        "srf_mha_attention: null pointer",
    ("srf_mha_attention_lse_ragged", "bad_length_and_Bt_65536"):
        "srf_mha_attention: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_lse_ragged", "bad_length_and_d_1025"):
        "srf_mha_attention_lse_ragged: example 1 has q_lengths[b] = 0 (allowed: 1..Lq = 9)",
    ("srf_mha_attention_bwd_ragged", "null_q"):
        "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)",
    ("srf_mha_attention_bwd_ragged", "null_lse"):
        "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)",
    ("srf_mha_attention_bwd_ragged", "null_workspace"):
        "srf_mha_attention_bwd: workspace is null (srf_mha_attention_bwd_workspace_bytes)",
    ("srf_mha_attention_bwd_ragged", "H_0"):
        "srf_mha_attention_bwd_ragged: bad sizes (H 0, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_bwd_ragged", "Bt_0"):
        "srf_mha_attention_bwd: bad sizes (Bt 0, H 2, d 16, Lq 9, Lk 7)",
    ("srf_mha_attention_bwd_ragged", "Bt_65536"):
        "srf_mha_attention_bwd: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_bwd_ragged", "example_2e31"):
        "srf_mha_attention_bwd: one example exceeds 2^31 elements",
    ("srf_mha_attention_bwd_ragged", "d_1025"):
        "srf_mha_attention_bwd: head dimension d = 1025 exceeds the generic kernel's 1024",
    ("srf_mha_attention_bwd_ragged", "bad_length"):
        "srf_mha_attention_bwd_ragged: example 1 has q_lengths[b] = 0 (allowed: 1..Lq = 9)",
    ("srf_mha_attention_bwd_ragged", "bad_length_and_null_q"):
        "srf_mha_attention_bwd: null input (q, k, v, o, lse or go)",
    ("srf_mha_attention_bwd_ragged", "bad_length_and_Bt_65536"):
        "srf_mha_attention_bwd: batch / heads too large (max 65535 each)",
    ("srf_mha_attention_bwd_ragged", "bad_length_and_d_1025"):
        "srf_mha_attention_bwd: head dimension d = 1025 exceeds the generic kernel's 1024",
}


@pytest.mark.parametrize("entry,case", [(e, c) for e in ENTRIES for c in CASES if applies(e, c)])
def test_refusal_is_the_recorded_one(entry, case):
    from sudo_rm_rf_amd import _lib
    assert call(_lib.load(), entry, case) == (-1, EXPECTED[entry, case])          # -1: SRF_EINVAL


def test_every_entry_has_every_case_that_applies_to_it():
    assert set(EXPECTED) == {(e, c) for e in ENTRIES for c in CASES if applies(e, c)}
    assert len(EXPECTED) == 54

"""Host-side checks of the attention backward's reach (N <= 640): what the library answers without a GPU, and that the header,
the ctypes table and the binary agree on the entry points the feature goes through."""
import ctypes
import os
import re

import slim_switch_moe_vit_amd as sm  # noqa: F401
from slim_switch_moe_vit_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slimmoe.h")


def test_attention_backward_reaches_640_tokens_at_head_dim_64():
    lib = _lib.load()
    for N in (1, 197, 256, 257, 577, 640):
        assert lib.smoe_attention_bwd_supported(N, 64) == 1, N
        assert lib.smoe_attention_supported(N, 64) == 1, N
    for N, hd in ((641, 64), (0, 64), (577, 32), (257, 128)):
        assert lib.smoe_attention_bwd_supported(N, hd) == 0, (N, hd)


def test_attention_entry_points_are_declared_exported_and_prototyped():
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(smoe_attention\w*)\s*\(", text))
    assert {"smoe_attention_supported", "smoe_attention_fwd", "smoe_attention_bwd_supported", "smoe_attention_bwd"} <= declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), f"libslimmoe_hip.so does not export {s}"
        assert s in _lib.SIGNATURES, f"_lib.SIGNATURES has no prototype for {s}"
    assert _lib.ABI_VERSION == 30 and _lib.load().smoe_abi_version() == 30
    # the header no longer limits lse / the backward to N <= 256
    doc = text[text.index("int smoe_attention_fwd("):text.index("int smoe_attention_bwd(")]
    assert "N <= 256)" not in doc and "N <= 640" in doc


def test_attention_backward_argument_checks_come_before_any_launch():
    lib = _lib.load()
    fake = 4096          # never dereferenced
    assert lib.smoe_attention_bwd(fake, fake, fake, fake, fake, 1, 0, 577, 16, 64, 0.125, None) == 0      # B == 0 returns at once
    assert lib.smoe_attention_bwd(fake, fake, fake, fake, fake, 1, 1, 641, 16, 64, 0.125, None) != 0
    assert b"N <= 640" in lib.smoe_last_error()
    assert lib.smoe_attention_bwd(fake, fake, fake, None, fake, 1, 1, 577, 16, 64, 0.125, None) != 0
    assert b"null" in lib.smoe_last_error()

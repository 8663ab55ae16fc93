"""The RotatE DIRECT kernels address the entity planes with 32-bit offsets
inside a descriptor that spans one 32-dim chunk plus 2 dims of look-ahead
(csrc/rotate.hip plane_chunk): a table whose span reaches 4 GiB
is refused with RNNL_ERR_INVALID before anything is launched (no GPU needed:
the argument check runs on the host and no pointer is dereferenced)."""
import ctypes

import pytest

from rnnlogic_amd import _native

MAX_E = 15790080  # 34 dims x 2 planes x ent_pad(E) x 4 bytes < 2^32


def test_direct_mode_refuses_a_chunk_span_of_4gib():
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    with pytest.raises(_native.NativeError) as ei:
        _native.call("rnnl_rotate_score_pieces", p, p, p, 1, 9.0, p, p, 1, MAX_E + 1, p, 0, _native.ROTATE_DIRECT,
                     p, 64, 1, 0.0, None)
    assert ei.value.code == _native.RNNL_ERR_INVALID
    assert "too large for the direct kernel" in str(ei.value)

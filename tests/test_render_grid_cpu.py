"""CPU: what dd_render_grid needs before a GPU sees it: the grid's shape is
the reference's (socket_server.py:165-166), the atlas header gained the label's
face without moving a byte of the three faces dd_render draws with, and the entry
point refuses bad grids with hipErrorInvalidValue before any launch."""
import ctypes
import hashlib
import math
import os
import re

import numpy as np
import pytest

from delivery_drone_amd import abi, grid_shape
from delivery_drone_amd.config import EnvConfig
from oracle import render as R
from render_grid_ref import compose, label_atlas, label_mask

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL_CHARS = " Game0123456789"
# The three faces as the parent commit's font_atlas.h held them: kHeight, kIndex, kOffset, kAdvance and the
# 32,837 coverage bytes, each as little-endian int64, concatenated, SHA-256.
FRAME_FACES_SHA256 = "2e0fe01e1414dcd599448d4374be49b6156a83a88b2c390363f4485dccfc74b0"
FRAME_GLYPHS, FRAME_BYTES = 113, 32837


def test_grid_shape_is_the_references():
    for k in range(1, 71):
        cols = math.ceil(math.sqrt(k))
        rows = math.ceil(k / cols)
        assert grid_shape(k) == (rows, cols), k
    assert grid_shape(7, 4) == (2, 4) and grid_shape(4, 1) == (4, 1) and grid_shape(3, cols=5) == (1, 5)
    for bad in ((0, None), (-1, None), (3, 0), (3, -2)):
        with pytest.raises(ValueError):
            grid_shape(*bad)


def test_the_frames_three_faces_are_unchanged():
    """The label's face went into tables of its own, so oracle.render.atlas()
    still reads exactly the parent's three faces."""
    height, index, offset, advance, cov = R.atlas()
    assert re.search(r"constexpr int kFaces = 3;", open(R._ATLAS_H).read())
    assert list(height) == [19, 24, 39] and len(index) == 3 * 128
    assert len(offset) == len(advance) == FRAME_GLYPHS and len(cov) == FRAME_BYTES
    parts = (height, index, offset, advance, cov)
    digest = hashlib.sha256(b"".join(np.asarray(a, dtype="<i8").tobytes() for a in parts)).hexdigest()
    assert digest == FRAME_FACES_SHA256
    assert sorted(g for g in index if g >= 0) == list(range(FRAME_GLYPHS))


def test_label_face_holds_the_labels_characters_and_nothing_else():
    height, index, offset, advance, cov = label_atlas()
    assert len(index) == 128
    have = "".join(chr(c) for c in range(128) if index[c] >= 0)
    assert sorted(have) == sorted(LABEL_CHARS)
    # its own numbering: glyphs 0..14 in the order of the tool's string, coverage cell after cell
    assert [int(index[ord(ch)]) for ch in LABEL_CHARS] == list(range(len(LABEL_CHARS)))
    assert len(offset) == len(advance) == len(LABEL_CHARS)
    assert [int(o) for o in offset] == [int(v) for v in np.concatenate(([0], np.cumsum(height * advance)[:-1]))]
    assert int(offset[-1] + height * advance[-1]) == len(cov)
    # DejaVu Sans Bold at 24 px (pygame's Font(None, 36)): taller than the HUD's 16 and 20 px, under the title's 33
    assert 24 < height < 39 and cov.max() == 255
    # the widest label a lane index can give fits the kernel's 256-column label box
    assert max(label_mask("Game " + str(d) * 10).shape[1] for d in range(10)) < 256  # int32: ten digits
    assert label_mask("Game 7").shape == (height, int(sum(advance[index[ord(c)]] for c in "Game 7")))
    assert label_mask("Game 7?").shape == label_mask("Game 7").shape  # no glyph: skipped, as text_mask does


def test_compose_pastes_tiles_and_clips_the_label_to_its_tile():
    H, W = 8, 16
    frames = [np.full((H, W, 3), 40 * (k + 1), dtype=np.uint8) for k in range(3)]
    plain = compose(frames, [5, 6, 7], 2, 2, labels=False)
    assert plain.shape == (2 * H, 2 * W, 3) and plain.dtype == np.uint8
    assert (plain[:H, :W] == 40).all() and (plain[:H, W:] == 80).all() and (plain[H:, :W] == 120).all()
    assert not plain[H:, W:].any()
    lab = compose(frames, [5, 6, 7], 2, 2)
    # the label's box starts at (10, 10) of the tile: rows 10.. do not exist in an 8-row tile, so nothing is drawn
    assert np.array_equal(lab, plain)
    tall = [np.full((40, W, 3), 40, dtype=np.uint8)]
    one = compose(tall + tall, [123456, None], 1, 2)
    changed = (one != 40).any(axis=2)
    assert changed[10:39, 10:W].any() and not changed[:, W:].any() and not changed[:10].any() and not changed[:, :10].any()


def _state(precision=abi.DD_F32):
    p = ctypes.c_void_p(1)
    return abi.DDState(p, p, p, p, p, p, p, p, p, p, p, p, p, 0, precision, 0)


def test_render_grid_argument_errors_without_gpu():
    lib = abi.lib()
    cfg = EnvConfig().to_abi()
    EINVAL = 1  # hipErrorInvalidValue
    st, rgb = _state(), ctypes.c_void_p(8)

    def grid(c=cfg, state=st, count=3, n=4, cols=2, rows=2, out=rgb, flags=7):
        return lib.dd_render_grid(ctypes.byref(c) if c is not None else None, ctypes.byref(state), None, None, count,
                                  n, cols, rows, out, flags, None)

    assert grid(cols=0) == EINVAL
    assert grid(rows=0) == EINVAL
    assert grid(cols=-1, rows=-4) == EINVAL
    assert grid(count=3, cols=2, rows=1) == EINVAL  # rows * cols < count
    assert grid(cols=256, rows=256) == EINVAL  # 65,536 tiles
    assert grid(cols=2 ** 31 - 1, rows=2 ** 31 - 1) == EINVAL  # the product is taken in 64 bits
    assert grid(out=None) == EINVAL
    assert grid(c=EnvConfig(world_width=802).to_abi()) == EINVAL  # rows are drawn 4 pixels at a time
    # everything dd_render refuses
    assert grid(c=None) == EINVAL
    assert grid(count=-1) == EINVAL
    assert grid(n=-1) == EINVAL
    assert grid(count=5, n=4, cols=3, rows=2) == EINVAL  # lanes 0..4 of a 4-lane batch
    assert grid(state=abi.DDState()) == EINVAL
    assert grid(state=_state(precision=7)) == EINVAL
    # count == 0 is a grid to black out, not a no-op: its arguments are checked like any other's
    assert grid(count=0, out=None) == EINVAL
    assert grid(count=0, cols=0) == EINVAL


def test_header_declares_the_entry_point_and_keeps_abi_13():
    text = open(os.path.join(REPO, "include", "dronestep.h")).read()
    assert re.search(r"#define DD_ABI_VERSION 13\b", text)
    assert abi.DD_ABI_VERSION == 13 and abi.lib().dd_abi_version() == 13
    assert re.search(r"DD_RENDER_LABELS = 4\b", text) and abi.DD_RENDER_LABELS == 4
    assert "dd_render_grid" in abi.EXPORTS and re.search(r"\bint dd_render_grid\(", text)

"""TEST INFRASTRUCTURE ONLY: numpy restatement of the composite grid of
``socket_server.py --render-all`` (:155-225) that dd_render_grid draws.

Every frame is pasted at (col * W, row * H) of a black surface, `cols` frames
to a row, and "Game {idx}" (pygame.font.Font(None, 36), yellow) is blended at
(x + 10, y + 10) with ``oracle.render._blend``.  The blend is done into a view
of the tile alone, which clips the label to its tile: the one departure of
dd_render_grid from pygame (render.hip's header).

The label's face is not one of the three that ``oracle.render.atlas()`` reads
(tests/test_render_cpu.py pins those tables to exactly three faces): it is the
kLabel* tables of the same header, parsed here the way the oracle parses its
own, and laid out by ``label_mask`` with ``oracle.render.text_mask``'s rule."""
import re

import numpy as np

from oracle import render as R

LABEL_AT = (10, 10)
_LABEL = None


def label_atlas():
    """(height, index[128], offset[g], advance[g], coverage bytes) of the label's face."""
    global _LABEL
    if _LABEL is None:
        src = open(R._ATLAS_H).read()

        def arr(name):
            m = re.search(r"\b" + name + r"\[[^\]]*\] = \{(.*?)\};", src, re.S)
            return np.array([int(t) for t in m.group(1).replace("\n", " ").split(",") if t.strip()], dtype=np.int64)

        height = int(re.search(r"constexpr int kLabelHeight = (\d+);", src).group(1))
        _LABEL = (height, arr("kLabelIndex"), arr("kLabelOffset"), arr("kLabelAdvance"), arr("kLabelAtlas"))
    return _LABEL


def label_mask(text: str):
    """Coverage image [h, w] of `text` in the label's face, laid out by summed
    advances; a character without a glyph is skipped (oracle.render.text_mask)."""
    h, index, offset, advance, cov = label_atlas()
    cols = []
    for ch in text:
        g = int(index[ord(ch) & 127])
        if g < 0:
            continue
        a = int(advance[g])
        cols.append(cov[offset[g]:offset[g] + h * a].reshape(h, a))
    return np.concatenate(cols, axis=1) if cols else np.zeros((h, 0), dtype=np.int64)


def compose(frames, lane_ids, rows, cols, labels=True):
    """uint8 [rows * H, cols * W, 3]: frames[k] ([H, W, 3]) as tile k, labelled
    with lane_ids[k]; an id of None leaves the tile unlabelled (not a lane)."""
    H, W = frames[0].shape[:2]
    assert len(frames) == len(lane_ids) <= rows * cols
    img = np.zeros((rows * H, cols * W, 3), dtype=np.int64)
    for k, (frame, lane) in enumerate(zip(frames, lane_ids)):
        r, c = divmod(k, cols)
        tile = img[r * H:(r + 1) * H, c * W:(c + 1) * W]
        tile[...] = frame
        if labels and lane is not None:
            R._blend(tile, label_mask(f"Game {int(lane)}"), LABEL_AT[0], LABEL_AT[1], R.YELLOW)
    return img.astype(np.uint8)

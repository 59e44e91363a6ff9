"""A minimal PNG writer for the image summaries (yolo_tf_amd/summary.py), and a reader for what it writes.

8 bits per sample, colour type 0 (grey), 2 (RGB) or 6 (RGBA) for depth 1, 3 or 4, no interlace, filter type 0 on every row -- so the pixel
data is ``zlib.decompress`` of the IDAT chunks with one zero byte in front of each row, and a test can read it with zlib alone.
TensorFlow's own PNG bytes are not reproducible (libpng's filter heuristics and zlib settings), so the compression level is free.
Host-side I/O only."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
COLOR_TYPE = {1: 0, 3: 2, 4: 6}
DEPTH = {v: k for k, v in COLOR_TYPE.items()}


def _chunk(kind, payload):
    return struct.pack('>I', len(payload)) + kind + payload + struct.pack('>I', zlib.crc32(kind + payload) & 0xffffffff)


def encode(image, level=6):
    """``image``: uint8 [H, W, depth] (or [H, W] for grey), depth 1, 3 or 4 -> PNG bytes."""
    image = np.ascontiguousarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in COLOR_TYPE, (image.dtype, image.shape)
    h, w, depth = image.shape
    assert h > 0 and w > 0
    rows = np.zeros((h, 1 + w * depth), np.uint8)          # filter type 0 in front of every row
    rows[:, 1:] = image.reshape(h, w * depth)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, COLOR_TYPE[depth], 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def decode(data):
    """Inverse of :func:`encode` for its own output (8-bit, colour type 0 / 2 / 6, filter 0, no interlace) -> uint8 [H, W, depth].
    Every chunk's CRC is checked."""
    if data[:8] != SIGNATURE:
        raise ValueError('not a PNG')
    i, header, idat, ended = 8, None, b'', False
    while i < len(data):
        n, kind = struct.unpack('>I', data[i:i + 4])[0], data[i + 4:i + 8]
        payload = data[i + 8:i + 8 + n]
        if struct.unpack('>I', data[i + 8 + n:i + 12 + n])[0] != zlib.crc32(kind + payload) & 0xffffffff:
            raise ValueError('bad CRC in chunk %r' % kind)
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', payload)
        elif kind == b'IDAT':
            idat += payload
        elif kind == b'IEND':
            ended = True
        i += 12 + n
    if header is None or not ended:
        raise ValueError('truncated PNG')
    w, h, bits, color, compression, filt, interlace = header
    if bits != 8 or color not in DEPTH or compression or filt or interlace:
        raise ValueError('not a PNG this module writes: %r' % (header,))
    depth = DEPTH[color]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    if raw.size != h * (1 + w * depth):
        raise ValueError('pixel data of %d bytes for a %d x %d x %d image' % (raw.size, h, w, depth))
    rows = raw.reshape(h, 1 + w * depth)
    if rows[:, 0].any():
        raise ValueError('a row filter other than 0')
    return rows[:, 1:].reshape(h, w, depth).copy()

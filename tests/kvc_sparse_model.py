"""A plain numpy model of KV regions that are backed only here and there: the reference of the far-offset GPU tests.

Per region a dict page_id -> uint8[page_bytes]. Every byte offset is a Python int, so no product in here can wrap; touching
a page that is not in the dict raises UnbackedError - the model is never asked about unbacked memory. Pinned against the
CPU oracle (okvc_compact_blocks) and the host-image expression of test_gpu_host_offload.py in test_sparse_model.py."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np


class UnbackedError(KeyError):
    pass


class SparseRegions:
    def __init__(self, n_regions: int, page_bytes: int):
        self.page_bytes = int(page_bytes)
        self.pages: List[Dict[int, np.ndarray]] = [dict() for _ in range(n_regions)]

    @property
    def n_regions(self) -> int:
        return len(self.pages)

    def load_page(self, r: int, page_id: int, data: np.ndarray) -> None:
        data = np.asarray(data, dtype=np.uint8)
        assert data.shape == (self.page_bytes,)
        self.pages[r][int(page_id)] = data.copy()

    def _page(self, r: int, page_id: int) -> np.ndarray:
        try:
            return self.pages[r][page_id]
        except KeyError:
            raise UnbackedError(f"region {r}: page {page_id} is not backed") from None

    def _pieces(self, off: int, n: int):
        """(page id, offset in the page, offset in the range, length) of the byte range [off, off + n)."""
        assert off >= 0 and n >= 0
        done = 0
        while done < n:
            p, o = divmod(off + done, self.page_bytes)
            k = min(self.page_bytes - o, n - done)
            yield p, o, done, k
            done += k

    def read(self, r: int, off: int, n: int) -> np.ndarray:
        out = np.empty(n, dtype=np.uint8)
        for p, o, at, k in self._pieces(int(off), int(n)):
            out[at:at + k] = self._page(r, p)[o:o + k]
        return out

    def write(self, r: int, off: int, data: np.ndarray) -> None:
        data = np.asarray(data, dtype=np.uint8).reshape(-1)
        pieces = list(self._pieces(int(off), data.size))
        for p, _, _, _ in pieces:
            self._page(r, p)             # all or nothing: raise before the first byte changes
        for p, o, at, k in pieces:
            self.pages[r][p][o:o + k] = data[at:at + k]

    def read_block(self, r: int, block_id: int, bb: int) -> np.ndarray:
        return self.read(r, int(block_id) * int(bb), bb)

    def write_block(self, r: int, block_id: int, bb: int, data: np.ndarray) -> None:
        assert np.asarray(data).size == bb
        self.write(r, int(block_id) * int(bb), data)

    def compact(self, src: Sequence[int], dst: Sequence[int], bb: int) -> None:
        """In every region copy block src[m] onto block dst[m], in list order."""
        assert len(src) == len(dst)
        for r in range(self.n_regions):
            for s, d in zip(src, dst):
                self.write_block(r, d, bb, self.read_block(r, s, bb))

    def image(self, ids: Sequence[int], bb: int) -> np.ndarray:
        """The block-major host image of copy_blocks_to_host: [block][region][bytes], flat."""
        out = np.empty((len(ids), self.n_regions, bb), dtype=np.uint8)
        for i, b in enumerate(ids):
            for r in range(self.n_regions):
                out[i, r] = self.read_block(r, b, bb)
        return out.reshape(-1)

    def scatter(self, image: np.ndarray, ids: Sequence[int], bb: int) -> None:
        """copy_blocks_from_host: image[i, r] becomes block ids[i] of region r."""
        img = np.asarray(image, dtype=np.uint8).reshape(len(ids), self.n_regions, bb)
        for i, b in enumerate(ids):
            for r in range(self.n_regions):
                self.write_block(r, b, bb, img[i, r])

    def backed(self):
        """(region, page id) of every backed page, in order."""
        return [(r, p) for r in range(self.n_regions) for p in sorted(self.pages[r])]

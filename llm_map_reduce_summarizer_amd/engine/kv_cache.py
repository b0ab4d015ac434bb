"""Paged KV cache sized for 288 GB of HBM per GPU.

Layout per layer: ``k``/``v`` [num_pages, Hkv, P, head_dim] bf16, i.e. a page
holds P consecutive positions of ONE kv head contiguously (16 KiB at P=64,
hd=128) -- the unit the decode-attention workgroups stream.  Page 0 is a
scratch page: idle decode slots point at it, real sequences never do.

``kv_dtype="fp8"``: ``k``/``v`` are uint8 [num_pages, Hkv, SLAB] byte slabs,
SLAB = P * hd + 4 * P -- the P rows of e4m3fn bytes then the P fp32 row scales
of one (page, kv head) (csrc/kernels/kv8.h): 8.25 KiB instead of 16 KiB, so a
decode step streams half the KV bytes and the cache holds ~1.94x the tokens.
``kv_dtype="fp8v"``: only ``v`` is fp8 slabs, ``k`` stays bf16 -- the scores'
K rounding is what peaked attention amplifies (a CPU emulation on the parity
checkpoint: K+V fp8 20 % logit error, V only 6 %, profiles/r4_fp8_kv_emulation.txt),
so this keeps 3/4 of the bf16 bytes at a third of the full variant's error.

Allocation is whole-sequence: a request reserves ceil((prompt + max_new) / P)
pages at admission, so a captured decode graph can run many steps without
the host touching block tables.  The free list is the native C++ allocator
(``csrc/runtime/page_alloc.cpp``) when built, else a Python list with the
same LIFO policy.
"""

from __future__ import annotations

import ctypes
import logging
import threading
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from ..ops._lib import runtime_lib

log = logging.getLogger("mrsum.kv")


class PageAllocator:
    """Reference-counted KV pages with a content index over full pages (csrc/runtime/page_alloc.cpp; the
    Python fallback below keeps the same policy, so both return the same ids for the same calls).

    ``alloc`` / ``free`` are the plain LIFO free list.  Prefix caching adds ``match`` (the cached pages
    that hold a prompt's head, one reference taken on each), ``publish`` (a sequence's full prompt pages
    become findable), ``release`` (= ``free``: one reference less; a published page nobody holds stays
    findable until ``alloc`` needs it, least recently used first) and ``reset`` (forget every node)."""

    PAGE_TOKENS = 64  # tokens of an indexed page (PAGE_TOKENS of page_alloc.cpp)

    def __init__(self, num_pages: int, native: Optional[bool] = None):
        """``native``: None = the native library when built, False = the Python fallback, True = required."""
        self.num_pages = num_pages
        self._lib = runtime_lib(required=bool(native)) if native is not False else None
        self._h = None
        if self._lib is not None and hasattr(self._lib, "mrsum_pages_create"):
            L = self._lib
            ip = ctypes.POINTER(ctypes.c_int)
            L.mrsum_pages_create.restype = ctypes.c_void_p
            L.mrsum_pages_create.argtypes = [ctypes.c_int, ctypes.c_int]
            L.mrsum_pages_alloc.restype = ctypes.c_int
            L.mrsum_pages_alloc.argtypes = [ctypes.c_void_p, ctypes.c_int, ip]
            L.mrsum_pages_free.restype = ctypes.c_int
            L.mrsum_pages_free.argtypes = [ctypes.c_void_p, ctypes.c_int, ip]
            L.mrsum_pages_available.restype = ctypes.c_int
            L.mrsum_pages_available.argtypes = [ctypes.c_void_p]
            L.mrsum_pages_destroy.argtypes = [ctypes.c_void_p]
            L.mrsum_pages_match.restype = ctypes.c_int
            L.mrsum_pages_match.argtypes = [ctypes.c_void_p, ip, ctypes.c_int, ip]
            L.mrsum_pages_publish.restype = ctypes.c_int
            L.mrsum_pages_publish.argtypes = [ctypes.c_void_p, ip, ctypes.c_int, ip, ctypes.c_int]
            L.mrsum_pages_release.restype = ctypes.c_int
            L.mrsum_pages_release.argtypes = [ctypes.c_void_p, ctypes.c_int, ip]
            L.mrsum_pages_reset.restype = None
            L.mrsum_pages_reset.argtypes = [ctypes.c_void_p]
            L.mrsum_pages_cached.restype = ctypes.c_int
            L.mrsum_pages_cached.argtypes = [ctypes.c_void_p]
            L.mrsum_pages_evictions.restype = ctypes.c_longlong
            L.mrsum_pages_evictions.argtypes = [ctypes.c_void_p]
            self._h = L.mrsum_pages_create(num_pages, 1)
        else:
            self._free = list(range(num_pages - 1, 0, -1))

    @property
    def native(self) -> bool:
        return self._h is not None

    # ---------------------------------------------------------------- Python fallback state
    def _ix(self) -> SimpleNamespace:
        """Reference counts and index of the fallback (made on first use from the free list)."""
        ix = self.__dict__.get("_index")
        if ix is None:
            refs = [1] * self.num_pages
            for i in self._free:
                refs[i] = 0
            # nodes: (parent page or -1, the page's token ids) -> page; evictable: page -> tick
            ix = self._index = SimpleNamespace(refs=refs, nodes={}, key={}, kids={}, tick={}, evictable={},
                                               clock=0, evictions=0, lock=threading.RLock())
        return ix

    def _drop(self, ix, root: int) -> int:
        """Forget node ``root`` and every node below it; pages nobody holds go back to the free list."""
        par = ix.key[root][0]
        if par >= 0:
            ix.kids[par].remove(root)
        stack, n = [root], 0
        while stack:
            i = stack.pop()
            stack.extend(ix.kids.pop(i, ()))
            del ix.nodes[ix.key.pop(i)]
            if ix.refs[i] == 0:
                del ix.evictable[i]
                self._free.append(i)
            n += 1
        return n

    # ---------------------------------------------------------------- the free list
    def available(self) -> int:
        """Pages an ``alloc`` can take: free ones and cached ones nobody holds."""
        if self._h is not None:
            return self._lib.mrsum_pages_available(self._h)
        ix = self.__dict__.get("_index")
        return len(self._free) + (len(ix.evictable) if ix is not None else 0)

    def alloc(self, n: int) -> List[int]:
        if n <= 0:
            return []
        if self._h is not None:
            buf = (ctypes.c_int * n)()
            if self._lib.mrsum_pages_alloc(self._h, n, buf) != 0:
                raise MemoryError("KV cache exhausted (%d pages requested, %d free)" % (n, self.available()))
            return list(buf)
        ix = self._ix()
        with ix.lock:
            if n > len(self._free) + len(ix.evictable):
                raise MemoryError("KV cache exhausted (%d pages requested, %d free)" % (n, self.available()))
            out = []
            for _ in range(n):
                if not self._free:  # least recently used evictable page, with the nodes below it
                    ix.evictions += self._drop(ix, min(ix.evictable, key=ix.evictable.get))
                i = self._free.pop()
                ix.refs[i] = 1
                out.append(i)
            return out

    def free(self, pages: List[int]) -> None:
        """Drop one reference per page (all or nothing; a page not held, or named twice, is refused)."""
        if not pages:
            return
        if self._h is not None:
            buf = (ctypes.c_int * len(pages))(*pages)
            if self._lib.mrsum_pages_free(self._h, len(pages), buf) != 0:
                raise ValueError("double free / bad page id")
            return
        ix = self._ix()
        with ix.lock:
            if len(set(pages)) != len(pages) or any(not 1 <= i < self.num_pages or ix.refs[i] <= 0 for i in pages):
                raise ValueError("double free / bad page id")
            for i in reversed(pages):
                ix.refs[i] -= 1
                if ix.refs[i] == 0:
                    if i in ix.key:
                        ix.evictable[i] = ix.tick[i]
                    else:
                        self._free.append(i)

    release = free

    # ---------------------------------------------------------------- the prefix index
    @staticmethod
    def _ids(tokens) -> np.ndarray:
        return np.ascontiguousarray(tokens, dtype=np.int32)

    def match(self, prompt) -> List[int]:
        """The longest cached chain of full pages that prefixes ``prompt``, at most (len - 1) // 64 pages (one
        token at least is always left to compute); takes a reference on each page returned."""
        P = self.PAGE_TOKENS
        cap = (len(prompt) - 1) // P if len(prompt) else 0
        if cap <= 0:
            return []
        if self._h is not None:
            t = self._ids(prompt)
            out = (ctypes.c_int * cap)()
            n = self._lib.mrsum_pages_match(self._h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(t), out)
            return list(out[:n])
        ix = self._ix()
        with ix.lock:
            t = self._ids(prompt)
            out, parent = [], -1
            while len(out) < cap:
                i = ix.nodes.get((parent, t[len(out) * P:(len(out) + 1) * P].tobytes()))
                if i is None:
                    break
                out.append(i)
                parent = i
            for i in reversed(out):  # leaf first: the head of a chain is its most recent page
                if ix.refs[i] == 0:
                    del ix.evictable[i]
                ix.refs[i] += 1
                ix.clock += 1
                ix.tick[i] = ix.clock
            return out

    def publish(self, prompt, pages: List[int], n_full: int) -> int:
        """Register the caller's first ``n_full`` pages (full of ``prompt``'s tokens, held by the caller) as the
        chain of ``prompt``.  A node that exists already stays, and the caller's page of that position stays
        private.  Returns the number of nodes added."""
        P = self.PAGE_TOKENS
        if n_full <= 0:
            return 0
        if n_full * P > len(prompt) or n_full > len(pages):
            raise ValueError("publish: %d full pages of a %d-token prompt holding %d pages"
                             % (n_full, len(prompt), len(pages)))
        t = self._ids(prompt)
        if self._h is not None:
            ip = ctypes.POINTER(ctypes.c_int)
            buf = (ctypes.c_int * n_full)(*pages[:n_full])
            n = self._lib.mrsum_pages_publish(self._h, t.ctypes.data_as(ip), len(t), buf, n_full)
            if n < 0:
                raise ValueError("publish: bad page id, or a page the caller does not hold")
            return n
        ix = self._ix()
        with ix.lock:
            if any(not 1 <= i < self.num_pages or ix.refs[i] <= 0 for i in pages[:n_full]):
                raise ValueError("publish: bad page id, or a page the caller does not hold")
            chain, parent, added = [], -1, 0
            for k in range(n_full):
                key = (parent, t[k * P:(k + 1) * P].tobytes())
                i = ix.nodes.get(key)
                if i is None:
                    i = pages[k]
                    if i in ix.key:  # the caller's page is another chain's node already: stop here
                        break
                    ix.nodes[key] = i
                    ix.key[i] = key
                    if parent >= 0:
                        ix.kids.setdefault(parent, []).append(i)
                    added += 1
                chain.append(i)
                parent = i
            for i in reversed(chain):
                ix.clock += 1
                ix.tick[i] = ix.clock
                if ix.refs[i] == 0:
                    ix.evictable[i] = ix.clock
            return added

    def reset(self) -> None:
        """Forget every node; pages with holders stay allocated until they are released."""
        if self._h is not None:
            self._lib.mrsum_pages_reset(self._h)
            return
        ix = self._ix()
        with ix.lock:
            for i in sorted(ix.key, reverse=True):
                if ix.refs[i] == 0:
                    self._free.append(i)
            ix.nodes.clear(), ix.key.clear(), ix.kids.clear(), ix.evictable.clear()

    def cached(self) -> int:
        """Nodes in the index."""
        if self._h is not None:
            return self._lib.mrsum_pages_cached(self._h)
        ix = self.__dict__.get("_index")
        return len(ix.key) if ix is not None else 0

    def evictions(self) -> int:
        """Nodes ``alloc`` has dropped from the index so far."""
        if self._h is not None:
            return int(self._lib.mrsum_pages_evictions(self._h))
        ix = self.__dict__.get("_index")
        return ix.evictions if ix is not None else 0

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                self._lib.mrsum_pages_destroy(self._h)
            except Exception:
                pass
            self._h = None


KV_DTYPES = ("bf16", "fp8", "fp8v")


class PagedKVCache:
    def __init__(self, n_layers: int, num_pages: int, n_kv_heads: int, page: int, head_dim: int,
                 dtype: torch.dtype, device: torch.device, kv_dtype: str = "bf16"):
        if num_pages < 2:
            raise ValueError("need at least 2 KV pages (page 0 is scratch)")
        if kv_dtype not in KV_DTYPES:
            raise ValueError("kv_dtype must be one of %s" % (KV_DTYPES,))
        if kv_dtype != "bf16" and (page, head_dim) != (64, 128):
            raise ValueError("the fp8 KV cache needs page 64 and head dim 128")
        self.page = page
        self.num_pages = num_pages
        self.kv_dtype = kv_dtype
        shape16, dt16 = (n_layers, num_pages, n_kv_heads, page, head_dim), dtype
        from ..ops.reference import kv8_slab
        shape8 = (n_layers, num_pages, n_kv_heads, kv8_slab(page, head_dim)) if kv_dtype != "bf16" else None
        kshape, kdt = (shape8, torch.uint8) if kv_dtype == "fp8" else (shape16, dt16)
        vshape, vdt = (shape8, torch.uint8) if kv_dtype in ("fp8", "fp8v") else (shape16, dt16)
        # zeroed, not empty: attention kernels read whole pages and mask the scores of rows past a
        # sequence's end (p = 0), and 0 x a stale NaN bit pattern in such a V row would still be NaN
        self.k = torch.zeros(kshape, dtype=kdt, device=device)
        self.v = torch.zeros(vshape, dtype=vdt, device=device)
        self.alloc = PageAllocator(num_pages)
        log.info("KV cache: %d pages x %d tokens (%.1f GiB)", num_pages, page,
                 (self.k.numel() * self.k.element_size() + self.v.numel() * self.v.element_size()) / 2 ** 30)

    def pages_for(self, n_tokens: int) -> int:
        return -(-n_tokens // self.page)

    @property
    def fp8(self) -> bool:
        """Any fp8 slab cache (K and V, or V only)."""
        return self.kv_dtype != "bf16"

    @staticmethod
    def size_pages(bytes_budget: int, n_layers: int, n_kv_heads: int, page: int, head_dim: int,
                   dtype_bytes: int = 2, kv_dtype: str = "bf16") -> int:
        bf, f8 = page * head_dim * dtype_bytes, page * head_dim + 4 * page
        per_head = {"bf16": 2 * bf, "fp8": 2 * f8, "fp8v": bf + f8}[kv_dtype]
        per_page = n_layers * n_kv_heads * per_head
        return max(2, bytes_budget // per_page)

"""Validity rules of the caches that carry state from one call to the next, on CPU tensors: the squared norms the encoder's
last conv leaves behind (ops._NormCache), the retrieval ranks of the last CLIPLoss forward (loss._cached_ranks) and the
content-keyed host->device tables (ops.UploadCache).  A stale hit in any of them changes a result without an error, so
every way a cached entry can go stale must miss."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------- ops._NormCache
def _norm_cache():
    from speech_decoding_amd.ops import _NormCache
    return _NormCache()


def test_norm_cache_hits_the_same_live_buffer_through_any_view():
    cache = _norm_cache()
    buf = torch.zeros(40, 8)
    norms = torch.arange(4.0)
    cache.put(buf, norms)
    assert cache.get(buf, 4) is norms
    assert cache.get(buf.detach().as_strided((40, 8), (8, 1), 0), 4) is norms     # what loss.as_rows hands to clip_forward


def test_norm_cache_misses_after_an_inplace_edit_through_a_view():
    cache = _norm_cache()
    buf = torch.zeros(40, 8)
    norms = torch.arange(4.0)
    cache.put(buf, norms)
    bview = buf.as_strided((4, 8, 10), (80, 1, 8), 0)       # a (B, C, T) view like ops.rows_view
    bview[2, 3, 4] = 1.0                                   # the owner itself is never touched by name
    assert cache.get(buf, 4) is None
    cache.put(buf, norms)
    col = buf[:, 5]                                         # a strided column view
    col.mul_(2.0)
    assert cache.get(buf.detach(), 4) is None


def test_norm_cache_misses_once_the_owner_is_freed_and_its_address_is_reused():
    cache = _norm_cache()
    arena = torch.zeros(64, 8)                             # keeps the memory alive: the address is reused deterministically
    owner = arena[:40]
    norms = torch.arange(4.0)
    cache.put(owner, norms)
    assert cache.get(arena[:40], 4) is norms               # owner alive, same storage and version: a hit
    del owner
    other = arena[:40]                                     # another tensor at the owner's address, same shape and version
    assert other.data_ptr() == arena.data_ptr()
    assert cache.get(other, 4) is None


def test_norm_cache_misses_after_a_shape_or_batch_size_change():
    cache = _norm_cache()
    arena = torch.zeros(64, 8)
    buf = arena[:40]
    norms = torch.arange(4.0)
    cache.put(buf, norms)
    assert cache.get(buf, 5) is None                       # batch size
    assert cache.get(buf, 3) is None
    assert cache.get(arena[:48], 4) is None                # more rows at the same address (another T)
    assert cache.get(arena[:32], 4) is None
    assert cache.get(buf, 4) is norms                      # the misses left the entry intact


def test_norm_cache_keeps_live_entries_when_it_prunes():
    cache = _norm_cache()
    keep = torch.zeros(10, 4)
    cache.put(keep, torch.ones(2))
    for _ in range(40):                                    # dead producers: pruned once there are more than 16 entries
        cache.put(torch.zeros(10, 4), torch.ones(2))
    assert len(cache.items) <= 18
    assert cache.get(keep, 2) is not None


# ---------------------------------------------------------------------------------------------------- loss rank cache
def _rank_cache():
    from speech_decoding_amd import loss
    return loss._cache_ranks, loss._cached_ranks


def test_rank_cache_hits_the_same_two_tensors_only():
    put, get = _rank_cache()
    Y, Z = torch.randn(12, 4, 5), torch.randn(12, 4, 5)
    cnt = torch.arange(12)
    put(Y, Z, cnt)
    assert get(Y, Z) is cnt
    assert get(Z, Y) is None
    assert get(Y, Z.clone()) is None                       # equal content, another tensor: the cache does not compare data


def test_rank_cache_misses_after_an_inplace_edit_through_a_view():
    put, get = _rank_cache()
    Y, Z = torch.randn(12, 4, 5), torch.randn(12, 4, 5)
    cnt = torch.arange(12)
    put(Y, Z, cnt)
    Z[:, 1].mul_(0.5)                                      # through a view of Z
    assert get(Y, Z) is None
    put(Y, Z, cnt)
    Y.as_strided((12, 20), (20, 1), 0)[3, 7] = 9.0         # through a view of Y
    assert get(Y, Z) is None


def test_rank_cache_misses_once_an_owner_is_freed_and_its_address_is_reused():
    put, get = _rank_cache()
    arena = torch.randn(24, 4, 5)
    Y, Z = torch.randn(12, 4, 5), arena[:12]
    put(Y, Z, torch.arange(12))
    del Z
    Z2 = arena[:12]                                        # same address, shape and version counter, another tensor
    assert get(Y, Z2) is None


def test_rank_cache_misses_after_a_shape_or_batch_size_change():
    put, get = _rank_cache()
    arena_y, arena_z = torch.randn(24, 4, 5), torch.randn(24, 4, 5)
    Y, Z = arena_y[:12], arena_z[:12]
    put(Y, Z, torch.arange(12))
    assert get(arena_y[:10], arena_z[:10]) is None         # ragged batch at the same addresses
    assert get(Y, arena_z[:12, :, :4]) is None             # another T
    assert get(Y, Z) is not None


# ---------------------------------------------------------------------------------------------------- ops.UploadCache
class _HostUpload:
    """The device upload replaced by a host copy: counts uploads, the cache's rules are what is tested."""

    def __init__(self):
        self.calls = 0

    def __call__(self, array, device):
        self.calls += 1
        return torch.from_numpy(np.array(array, copy=True))


def _upload_cache(capacity):
    from speech_decoding_amd.ops import UploadCache
    up = _HostUpload()
    return UploadCache(capacity=capacity, upload=up), up


def test_upload_cache_returns_the_same_tensor_only_for_equal_content_and_dtype():
    cache, up = _upload_cache(8)
    a = np.array([1, 2, 3, 4], dtype=np.int32)
    t = cache.upload("k", a, "dev")
    assert cache.upload("k", a.copy(), "dev") is t and up.calls == 1        # equal content, another array
    b = a.copy()
    b[3] = 5
    tb = cache.upload("k", b, "dev")                                         # one element differs
    assert tb is not t and torch.equal(tb, torch.from_numpy(b))
    tf = cache.upload("k", a.view(np.float32), "dev")                       # the same bytes as another dtype
    assert tf is not t and tf.dtype == torch.float32
    assert cache.upload("k", a.reshape(2, 2), "dev") is not t                # the same bytes in another shape
    assert cache.upload("other", a, "dev") is not t                          # another key
    assert cache.upload("k", a, "dev2") is not t                             # another device
    assert cache.upload("k", a, "dev") is t
    src = a.copy()
    t2 = cache.upload("m", src, "dev")
    src[0] = 99                                                              # the caller reusing its host array
    assert cache.upload("m", src, "dev") is not t2
    assert torch.equal(t2, torch.from_numpy(a))                              # the first upload kept its content


def test_upload_cache_evicts_in_lru_order_at_capacity():
    cache, up = _upload_cache(3)
    arrs = [np.full(4, i, dtype=np.int32) for i in range(5)]
    t = [cache.upload("k", a, "dev") for a in arrs[:3]]
    assert cache.upload("k", arrs[0], "dev") is t[0]                         # 0 becomes the most recently used
    cache.upload("k", arrs[3], "dev")                                        # evicts 1, the least recently used
    assert len(cache.items) == 3
    assert cache.upload("k", arrs[0], "dev") is t[0]
    assert cache.upload("k", arrs[2], "dev") is t[2]
    n = up.calls
    t1 = cache.upload("k", arrs[1], "dev")                                   # gone: uploaded again, evicting 3
    assert t1 is not t[1] and up.calls == n + 1
    assert cache.upload("k", arrs[0], "dev") is t[0] and cache.upload("k", arrs[2], "dev") is t[2]
    n = up.calls
    cache.upload("k", arrs[3], "dev")
    assert up.calls == n + 1

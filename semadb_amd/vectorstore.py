"""Mirror of the quantizers of shard/vectorstore over the C ABI: product.go (K5, K6, K8) and binary.go.

The plain store's device form is the index slab itself (vamana.IndexVamana.load / distance_batch);
this module carries the quantizer: newProductQuantizer (product.go:42-88), Fit (:175-236), encode
(:136-159), DistanceFromFloat (:238-277) and DistanceFromPoint (:279-305) in batched form; and the binary
quantizer's threshold, Fit (binary.go:145-185), encode (:103-129) and bit distances (distance.go:45-67).
"""
import ctypes as C

import numpy as np

from . import _buf
from ._lib import BIT_METRICS, MEM_HOST, METRICS, SemaDBError, check, lib


class ProductQuantizerParameters:
    """models.ProductQuantizerParameters (models/quantizer.go:51-63)"""

    def __init__(self, NumCentroids, NumSubVectors, TriggerThreshold=10000):
        self.NumCentroids, self.NumSubVectors, self.TriggerThreshold = NumCentroids, NumSubVectors, TriggerThreshold


class ProductQuantizer:
    def __init__(self, distFnName, params: ProductQuantizerParameters, vectorLen, device=0):
        if distFnName not in METRICS:  # product.go:48-50
            raise SemaDBError(1, "distance function %s not supported for product quantisation" % distFnName)
        self.params, self.vectorLen, self.device = params, vectorLen, device
        h = C.c_void_p()
        check(lib().sdb_pq_create(vectorLen, METRICS[distFnName], params.NumSubVectors, params.NumCentroids, device,
                                  C.byref(h)))
        self._h = h
        self.M, self.K = params.NumSubVectors, params.NumCentroids
        self.subVectorLen = vectorLen // params.NumSubVectors

    def close(self):
        if getattr(self, "_h", None):
            lib().sdb_pq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Fit(self, X, first_idx, alias=True):
        """productQuantizer.Fit (product.go:175-236) over the rows of X in the given order; returns codes."""
        assert isinstance(X, np.ndarray) and X.dtype == np.float32 and X.flags.c_contiguous
        fi = np.ascontiguousarray(first_idx, dtype=np.uint32)
        assert fi.size == self.M
        codes = np.zeros((X.shape[0], self.M), dtype=np.uint8)
        check(lib().sdb_pq_fit(self._h, _buf.np_ptr(X), X.shape[0], _buf.np_ptr(fi), 1 if alias else 0,
                               _buf.np_ptr(codes), MEM_HOST, None))
        return codes

    def set_codebook(self, flat_centroids):
        fc = np.ascontiguousarray(flat_centroids, dtype=np.float32)
        assert fc.size == self.M * self.K * self.subVectorLen
        check(lib().sdb_pq_set_codebook(self._h, _buf.np_ptr(fc), MEM_HOST))

    def codebook(self):
        fc = np.zeros((self.M, self.K, self.subVectorLen), dtype=np.float32)
        cd = np.zeros((self.M, self.K, self.K), dtype=np.float32)
        check(lib().sdb_pq_get_codebook(self._h, _buf.np_ptr(fc), _buf.np_ptr(cd)))
        return fc, cd

    def encode(self, vectors):
        k, vp, mem, shape = _buf.as_f32(vectors)
        codes, cp = _buf.empty_like_mem(mem, (shape[0], self.M), "uint8", self.device)
        check(lib().sdb_pq_encode(self._h, vp, shape[0], cp, mem, _buf.current_stream(mem)))
        return codes

    def lut_distance(self, queries, codes):
        """DistanceFromFloat batched: out[q, c] (product.go:250-277)"""
        k, qp, mem, qs = _buf.as_f32(queries)
        if mem == MEM_HOST:
            cd = np.ascontiguousarray(codes, dtype=np.uint8)
            cptr, nc = _buf.np_ptr(cd), cd.shape[0]
        else:
            cd = codes.contiguous()
            cptr, nc = C.c_void_p(cd.data_ptr()), cd.shape[0]
        out, op = _buf.empty_like_mem(mem, (qs[0], nc), "float32", self.device)
        check(lib().sdb_pq_lut_distance(self._h, qp, qs[0], cptr, nc, op, mem, _buf.current_stream(mem)))
        return out

    def sym_distance(self, codes_x, codes_y):
        """DistanceFromPoint batched over pairs (product.go:293-304)"""
        cx = np.ascontiguousarray(codes_x, dtype=np.uint8)
        cy = np.ascontiguousarray(codes_y, dtype=np.uint8)
        out = np.zeros(cx.shape[0], dtype=np.float32)
        check(lib().sdb_pq_sym_distance(self._h, _buf.np_ptr(cx), _buf.np_ptr(cy), cx.shape[0], _buf.np_ptr(out),
                                        MEM_HOST, None))
        return out


def attach(index, pq: ProductQuantizer, ids=None, codes=None):
    """Switch a vamana.IndexVamana to the fitted quantizer (what a fitted productQuantizer store does).
    Every stored vector is encoded; `ids`/`codes` then overwrite the centroid ids of those points -- the
    k-means labels Fit leaves on its training points (product.go:216-218) or codes read back from a bucket."""
    check(lib().sdb_index_attach_pq(index._h, pq._h, None))
    index._pq = pq  # keep alive
    if ids is not None:
        set_codes(index, ids, codes)


def set_codes(index, ids, codes):
    ids_a = np.ascontiguousarray(ids, dtype=np.uint64)
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    assert cd.shape == (ids_a.size, index._pq.M)
    check(lib().sdb_index_set_codes(index._h, ids_a.size, _buf.np_ptr(ids_a), _buf.np_ptr(cd)))


def get_codes(index, ids):
    ids_a = np.ascontiguousarray(ids, dtype=np.uint64)
    cd = np.zeros((ids_a.size, index._pq.M), dtype=np.uint8)
    check(lib().sdb_index_get_codes(index._h, ids_a.size, _buf.np_ptr(ids_a), _buf.np_ptr(cd)))
    return cd


class BinaryQuantizerParameters:
    """models.BinaryQuantizerParamaters (models/quantizer.go:30-49).  Threshold None = not set (the reference's nil
    pointer): the threshold is then fitted as the column means once TriggerThreshold points are stored."""

    def __init__(self, Threshold=None, TriggerThreshold=0, DistanceMetric="hamming"):
        self.Threshold, self.TriggerThreshold, self.DistanceMetric = Threshold, TriggerThreshold, DistanceMetric

    def Validate(self):
        if self.Threshold is None and (self.TriggerThreshold < 0 or self.TriggerThreshold > 50000):  # quantizer.go:42-44
            raise SemaDBError(1, "triggerThreshold must be between 0 and 50000, got %d" % self.TriggerThreshold)
        if self.DistanceMetric not in BIT_METRICS:  # :45-47
            raise SemaDBError(1, "invalid distance metric for binary quantization, got %s" % self.DistanceMetric)


class BinaryQuantizer:
    """binaryQuantizer (binary.go:25-64) without its bucket: the threshold and the bit distance function"""

    def __init__(self, params: BinaryQuantizerParameters, vectorLen, device=0):
        if params.DistanceMetric not in BIT_METRICS:  # distance.go:91-93
            raise SemaDBError(1, "failed to get bit distance function: unknown bit distance function: %s"
                              % params.DistanceMetric)
        self.params, self.vectorLen, self.device = params, vectorLen, device
        self.metric = BIT_METRICS[params.DistanceMetric]
        self.W = (vectorLen + 63) // 64  # binary.go:107-111
        h = C.c_void_p()
        check(lib().sdb_bq_create(vectorLen, self.metric, device, C.byref(h)))
        self._h = h
        if params.Threshold is not None:  # binary.go:51-56
            self.set_threshold(np.full(vectorLen, params.Threshold, dtype=np.float32))

    def close(self):
        if getattr(self, "_h", None):
            lib().sdb_bq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_threshold(self, thr):
        """a threshold read from the bucket (binary.go:58-61), one float per element"""
        t = np.ascontiguousarray(thr, dtype=np.float32)
        assert t.shape == (self.vectorLen,)
        check(lib().sdb_bq_set_threshold(self._h, _buf.np_ptr(t), MEM_HOST))

    def threshold(self):
        """what Flush stores (binary.go:240-242); None while the quantizer has no threshold"""
        t = np.zeros(self.vectorLen, dtype=np.float32)
        is_set = C.c_int(0)
        check(lib().sdb_bq_get_threshold(self._h, _buf.np_ptr(t), C.byref(is_set)))
        return t if is_set.value else None

    def Fit(self, X):
        """binaryQuantizer.Fit's first pass (binary.go:152-173) over the rows of X in the given order; a quantizer
        that has a threshold keeps it (:148).  Whether enough points are stored (TriggerThreshold) is the caller's
        business."""
        k, xp, mem, shape = _buf.as_f32(X)
        assert len(shape) == 2 and shape[1] == self.vectorLen
        check(lib().sdb_bq_fit(self._h, xp, shape[0], mem, _buf.current_stream(mem)))

    def encode(self, vectors):
        """codes [n][W] uint64 (int64 for a device tensor: torch has no unsigned 64-bit type; same bits)"""
        k, vp, mem, shape = _buf.as_f32(vectors)
        assert len(shape) == 2 and shape[1] == self.vectorLen
        codes, cp = _buf.empty_like_mem(mem, (shape[0], self.W), "uint64", self.device)
        check(lib().sdb_bq_encode(self._h, vp, shape[0], cp, mem, _buf.current_stream(mem)))
        return codes

    def distance(self, qcodes, ccodes):
        """bitDistFn batched: out[q, c] (distance.go:45-67)"""
        return bit_distance(self.params.DistanceMetric, qcodes, ccodes, self.device)


def bit_distance(distFnName, qcodes, ccodes, device=0):
    """distance.GetBitDistanceFn(name) batched over two arrays of codes [nq][W], [nc][W] -> out[nq, nc]"""
    if distFnName not in BIT_METRICS:
        raise SemaDBError(1, "unknown bit distance function: %s" % distFnName)
    if _buf.is_torch_cuda(qcodes):
        q, c = qcodes.contiguous(), ccodes.contiguous()
        mem, qp, cp = 1, C.c_void_p(q.data_ptr()), C.c_void_p(c.data_ptr())
    else:
        q, c = np.ascontiguousarray(qcodes, dtype=np.uint64), np.ascontiguousarray(ccodes, dtype=np.uint64)
        mem, qp, cp = MEM_HOST, _buf.np_ptr(q), _buf.np_ptr(c)
    assert q.ndim == 2 and c.ndim == 2 and q.shape[1] == c.shape[1]
    out, op = _buf.empty_like_mem(mem, (q.shape[0], c.shape[0]), "float32", device)
    check(lib().sdb_bit_distance_batch(BIT_METRICS[distFnName], q.shape[1], qp, q.shape[0], cp, c.shape[0], op, mem,
                                       device, _buf.current_stream(mem)))
    return out


def attach_binary(index, bq: BinaryQuantizer):
    """Switch a vamana.IndexVamana to the binary quantizer (what a binaryQuantizer store with a threshold does).  A
    quantizer without a threshold is fitted from the index's stored rows first (binary.go:145-185)."""
    check(lib().sdb_index_attach_bq(index._h, bq._h, None))
    index._bq = bq  # keep alive


def _code_words(index):
    """words per code row of an index: an attached quantizer has the index's own length (sdb_index_attach_bq), so the
    width is known with nothing attached too, and the library answers that case itself (SDB_ERR_STATE)"""
    return (index.parameters.VectorSize + 63) // 64


def set_bit_codes(index, ids, codes):
    ids_a = np.ascontiguousarray(ids, dtype=np.uint64)
    cd = np.ascontiguousarray(codes, dtype=np.uint64)
    assert cd.shape == (ids_a.size, _code_words(index))
    check(lib().sdb_index_set_bit_codes(index._h, ids_a.size, _buf.np_ptr(ids_a), _buf.np_ptr(cd)))


def get_bit_codes(index, ids):
    ids_a = np.ascontiguousarray(ids, dtype=np.uint64)
    cd = np.zeros((ids_a.size, _code_words(index)), dtype=np.uint64)
    check(lib().sdb_index_get_bit_codes(index._h, ids_a.size, _buf.np_ptr(ids_a), _buf.np_ptr(cd)))
    return cd


QuantizerNone, QuantizerBinary, QuantizerProduct = "none", "binary", "product"


class Quantizer:
    """models.Quantizer (models/quantizer.go:5-28)"""

    def __init__(self, Type=QuantizerNone, Product: ProductQuantizerParameters = None,
                 Binary: BinaryQuantizerParameters = None):
        self.Type, self.Product, self.Binary = Type, Product, Binary


def New(params, distFnName, vectorLength, device=0):
    """vectorstore.New (vectorstore.go:47-96): None for the plain store (the index slab), a BinaryQuantizer for
    `binary`, a ProductQuantizer for `product`."""
    if distFnName in BIT_METRICS:
        # a collection whose own metric is a bit metric: 0.0 / 1.0 vectors cut at 0.5 (vectorstore.go:51-66)
        params = Quantizer(QuantizerBinary, Binary=BinaryQuantizerParameters(Threshold=0.5, DistanceMetric=distFnName))
    elif distFnName not in METRICS:
        raise SemaDBError(1, "unknown float32 distance function: %s" % distFnName)
    if params is None or params.Type == QuantizerNone:
        return None
    if params.Type == QuantizerBinary:
        if params.Binary is None:
            raise SemaDBError(1, "binary quantizer parameters are nil")
        return BinaryQuantizer(params.Binary, vectorLength, device)
    if params.Type != QuantizerProduct:
        raise SemaDBError(1, "unknown vector store type %s" % params.Type)
    if params.Product is None:
        raise SemaDBError(1, "product quantizer parameters are nil")
    pp = params.Product
    if vectorLength % pp.NumSubVectors != 0:  # product.go:44-46
        raise SemaDBError(1, "vector length %d must be divisible by num subvectors %d" % (vectorLength, pp.NumSubVectors))
    if pp.NumCentroids > 256:  # product.go:63-65
        raise SemaDBError(1, "number of centroids %d cannot exceed 256" % pp.NumCentroids)
    return ProductQuantizer(distFnName, pp, vectorLength, device)

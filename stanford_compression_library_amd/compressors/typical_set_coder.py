"""Typical-set coding with the reference's class API: a block is cut into chunks of ``n`` symbols; a chunk of the typical set
is coded as ``0`` and its index there, any other chunk as ``1`` and its index in ``X^n``.

Drop-in for reference scl/compressors/typical_set_coder.py: ``compute_normalized_negative_log_prob_chunk``, ``is_typical``,
``TypicalSetCoderParams``, ``generate_typical_set_coder_lookup_tables``, ``TypicalSetEncoder`` / ``TypicalSetDecoder``.

The reference enumerates ``X^n`` in Python in both constructors.  Here the constructors build the tables on the device
(``backend.models.TypicalSetModel``, csrc/scl_typical.hip: a classification of all ``K^n`` tuples and a prefix count), and
``index_typical`` / ``index_overall`` / ``inverse_index_*`` are views of those tables, built on first use.  A tuple is typical
by the reference's float rule, operation for operation (csrc/scl_typical_rule.h), so the bits are the
reference's.  Symbols travel as their positions in ``prob_dist.alphabet``, uint16 above 256 symbols.

There is no host path for small blocks: every block goes to the device, and the constructors need one (``SclHipError``
without).  ``K^n`` above 2^24 tuples or more than 65 536 symbols raise ``NotImplementedError``.

Errors follow the reference where it has a defined one -- an unknown symbol and a typical index outside the set are
``KeyError``, a block that is no whole number of chunks ``AssertionError``; a stream cut inside its last codeword, a flag 0
with an empty typical set and an overall index of ``K^n`` and more are ``SclHipError`` with the chunk status (the reference
reads past the end, hits a ``TypeError`` on ``None`` or a ``KeyError`` that is an accident of its dicts).
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from ..backend import lib as _lib
from ..backend.models import TypicalSetModel
from ..core.data_block import DataBlock
from ..core.data_encoder_decoder import DataDecoder, DataEncoder
from ..core.prob_dist import ProbabilityDist
from ..utils.bitarray_utils import BitArray
from ._uint_block import truncated

__all__ = ["compute_normalized_negative_log_prob_chunk", "is_typical", "TypicalSetCoderParams",
           "generate_typical_set_coder_lookup_tables", "TypicalSetEncoder", "TypicalSetDecoder", "MAX_TUPLES", "MAX_ALPHABET"]

MAX_TUPLES = TypicalSetModel.MAX_TUPLES  # K^n: the longest codeword is then 25 bits, the rank table 64 MiB
MAX_ALPHABET = 1 << 16                   # uint16 symbol indices


def compute_normalized_negative_log_prob_chunk(chunk, prob_dist: ProbabilityDist):
    """-log2 P(chunk) / len(chunk), summed in sequence order"""
    log_prob = 0
    for symbol in chunk:
        log_prob += prob_dist.neg_log_probability(symbol)
    return log_prob / len(chunk)


def is_typical(chunk, prob_dist: ProbabilityDist, eps):
    """is the chunk within ``eps`` of the entropy?"""
    return np.abs(compute_normalized_negative_log_prob_chunk(chunk, prob_dist) - prob_dist.entropy) <= eps


@dataclass
class TypicalSetCoderParams:
    n: int                       # the chunk size
    eps: float                   # a chunk is typical if its normalised -log2 probability is within eps of the entropy
    prob_dist: ProbabilityDist   # the distribution that defines the typical chunks

    def __init__(self, n: int, eps: float, prob_dist: ProbabilityDist):
        self.n = n
        self.eps = eps
        self.prob_dist = prob_dist


def generate_typical_set_coder_lookup_tables(params: TypicalSetCoderParams):
    """(index_typical, index_overall) by the host rule, tuple by tuple in Python: kept for callers of the reference's
    function; the classes do not use it"""
    index_typical, index_overall = {}, {}
    for t, chunk in enumerate(itertools.product(params.prob_dist.alphabet, repeat=params.n)):
        if is_typical(chunk, params.prob_dist, params.eps):
            index_typical[chunk] = len(index_typical)
        index_overall[chunk] = t
    return index_typical, index_overall


def model_inputs(params: TypicalSetCoderParams):
    """-> (nlp[K] float64, entropy) as the reference computes them: numpy's log2 per symbol, the entropy summed in
    alphabet order"""
    dist = params.prob_dist
    nlp = np.array([dist.neg_log_probability(s) for s in dist.alphabet], dtype=np.float64)
    return nlp, float(dist.entropy)


class _TypicalSetCoder:
    """what the encoder and the decoder share: the device model and the views of its tables"""

    def __init__(self, params: TypicalSetCoderParams) -> None:
        self.params = params
        alphabet = params.prob_dist.alphabet
        K, n = len(alphabet), int(params.n)
        if K > MAX_ALPHABET:
            raise NotImplementedError(f"alphabet of {K} symbols: the device carries symbol indices of 16 bits, "
                                      f"at most {MAX_ALPHABET} symbols")
        tuples = 1 if K <= 1 else (K ** n if 0 <= n <= 24 else MAX_TUPLES + 1)  # (2^24 has no tuple longer than 24)
        if tuples > MAX_TUPLES:
            raise NotImplementedError(f"{K}^{n} tuples: the device enumerates at most 2^24 = {MAX_TUPLES} (a codeword of 25 "
                                      "bits, a rank table of 64 MiB)")
        nlp, entropy = model_inputs(params)
        self._model = TypicalSetModel(nlp, n, entropy, params.eps)
        self._alphabet = alphabet
        self._views = {}
        self.index_bitlen_typical = self._model.bt  # None: an empty typical set
        self.index_bitlen_overall = self._model.bo

    def _chunk(self, t: int) -> Tuple:
        K, digits = len(self._alphabet), []
        for _ in range(self._model.n):
            t, x = divmod(t, K)
            digits.append(self._alphabet[x])
        return tuple(reversed(digits))

    def _view(self, name: str):
        """the four dicts of the reference, from the device tables, on first use"""
        if name not in self._views:
            if name in ("index_typical", "inverse_index_typical"):
                _, inv = self._model.tables()
                chunks = [self._chunk(int(t)) for t in inv]
            else:
                chunks = list(itertools.product(self._alphabet, repeat=self._model.n))
            forward = name.startswith("index")
            self._views[name] = {c: i for i, c in enumerate(chunks)} if forward else dict(enumerate(chunks))
        return self._views[name]

    @property
    def index_typical(self):
        return self._view("index_typical")

    @property
    def index_overall(self):
        return self._view("index_overall")


class TypicalSetEncoder(_TypicalSetCoder, DataEncoder):
    def __init__(self, params: TypicalSetCoderParams) -> None:
        super().__init__(params)
        self._index_of = {s: i for i, s in enumerate(self._alphabet)}

    def encode_block(self, data_block: DataBlock) -> BitArray:
        assert data_block.size % self.params.n == 0, "Input to typical set encoder should be multiple of chunk length n"
        data = data_block.data_list
        if not data:
            return BitArray("")
        idx = np.fromiter(map(self._index_of.__getitem__, data), dtype=self._model.sym_dtype, count=len(data))  # KeyError
        packed, nbits, status = self._model.encode_host(idx)
        if status:
            raise _lib.SclHipError(_lib.E_CHUNK, "scl_typical_encode_block_host", f"block status 0x{status:x}")
        return BitArray.from_packed(packed, nbits)


class TypicalSetDecoder(_TypicalSetCoder, DataDecoder):
    @property
    def inverse_index_typical(self):
        return self._view("inverse_index_typical")

    @property
    def inverse_index_overall(self):
        return self._view("inverse_index_overall")

    def decode_block(self, encoded_bitarray: BitArray):
        """-> (DataBlock, num_bits_consumed): the whole of ``encoded_bitarray`` is the block, as in the reference"""
        nbits = len(encoded_bitarray)
        if nbits == 0:
            return DataBlock([]), 0
        what = "scl_typical_decode_block_host"
        idx, used, status = self._model.decode_host(encoded_bitarray.packed(), nbits)
        if status & _lib.ST_TRUNCATED:
            raise truncated(what)
        if status & _lib.ST_STATE and self._model.bt is not None and int(encoded_bitarray._b[used]) == 0:
            bt = self._model.bt
            raise KeyError(int("0" + "".join(map(str, encoded_bitarray._b[used + 1: used + 1 + bt].tolist())), 2))
        if status:
            raise _lib.SclHipError(_lib.E_CHUNK, what, f"{what}: chunk status 0x{status:x}"
                                   + (" STATE" if status & _lib.ST_STATE else ""))
        return DataBlock(list(map(self._alphabet.__getitem__, idx.tolist()))), used

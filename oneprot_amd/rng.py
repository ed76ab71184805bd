"""The host side of the counter-based random streams (device side: csrc/philox.h): the domain table, the stream-id layout, the process-wide tower numbering
and the state every stream owner carries.  A stream id is the high counter words of Philox4x32-10 (the key is the seed): bits 60..63 the DOMAIN (the purpose of
the draw, so that no two consumers can draw the same mask), bits 44..59 the TOWER (construction order within the process until OneProtLitModule re-numbers it by
modality name; saved / restored with the stream state), bits 0..43 the consumer's own (call, layer, site) numbering.  A consumer with no tower (gbt.py) has a
60-bit local field."""
import itertools

import torch

DOMAINS = {"bert": 1, "lora": 2, "msa": 3, "pronet": 4, "probe": 5, "gbt": 6}      # a new consumer takes the next number HERE
assert len(set(DOMAINS.values())) == len(DOMAINS) and all(0 < v < 16 for v in DOMAINS.values())
FIXED_SEED = 0x5EED0000            # + tower id: the probe's and ProNet's seed, which does not follow torch.manual_seed

_uids = itertools.count()


def stream_id(domain, uid, local):
    """uid None: the tower-less form"""
    if uid is None:
        return (int(domain) << 60) | (int(local) & ((1 << 60) - 1))
    return (int(domain) << 60) | (int(uid) << 44) | (int(local) & ((1 << 44) - 1))


def next_uid():
    """one numbering of the towers of a process, in construction order"""
    return next(_uids) & 0xFFFF


class StreamOwner:
    """Mixin of a module that owns streams.  The state is plain attributes on the owner: _rng_uid, and per stream family a seed and a call counter
    (_drop_seed / _drop_calls, _lora_seed / _lora_calls), absent until the family is seeded."""

    def _init_streams(self, fixed_seed=False):
        self._rng_uid = next_uid()
        if fixed_seed:
            self._drop_seed, self._drop_calls = FIXED_SEED + self._rng_uid, 0

    def _seed_streams(self, family="_drop"):
        """masks follow torch.manual_seed; every call / layer / site draws its own stream"""
        setattr(self, family + "_seed", int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF)
        setattr(self, family + "_calls", 0)

    def _next_call(self, family="_drop"):
        """the id of this call (its own masks; a backward regenerates them from (seed, call, ...)); seeds the family on first use"""
        if getattr(self, family + "_seed", None) is None:
            self._seed_streams(family)
        call = getattr(self, family + "_calls")
        setattr(self, family + "_calls", call + 1)
        return call

    def _rng_stream(self, domain, local):
        return stream_id(domain, self._rng_uid, local)

    def rng_state(self):
        """Seeds and call counters of the streams (plain ints): what a checkpoint has to carry for a resumed run to continue the mask
        sequence instead of replaying it from call 0 (OneProtLitModule.on_save_checkpoint / on_load_checkpoint)."""
        st = {k: int(getattr(self, k)) for k in ("_lora_seed", "_lora_calls", "_drop_seed", "_drop_calls") if getattr(self, k, None) is not None}
        if st:
            st["_rng_uid"] = int(self._rng_uid)              # the tower id inside the stream ids: a resumed process continues THESE streams
        return st

    def set_rng_state(self, state):
        for k in ("_lora_seed", "_lora_calls", "_drop_seed", "_drop_calls", "_rng_uid"):
            if k in state:
                setattr(self, k, int(state[k]))

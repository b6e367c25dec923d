"""Training-data feeder of the WaveNet vocoder.

Same on-disk contract and batch tensors as the reference's ``wavenet_vocoder/feeder.py``:
  * ``map.txt`` lines ``audio_path|mel_path|gta_mel_path|speaker_id|...`` (columns 0..3 are read; the GTA column
    is used when ``hparams.train_with_GTA``), ``audio-*.npy`` float32 [T] (int16 class ids for mulaw-quantize),
    ``mel-*.npy`` float32 [Tc, num_mels] in [-max_abs_value, max_abs_value], with T == Tc * hop_size;
  * train/test split with sklearn (``random_state = wavenet_data_random_state``), 64-batch groups sorted by
    length, hop-aligned random crops to ``max_time_steps``, mel padding with the silence value followed by
    the [0,1] normalisation.
Differences (by design): batches are produced as device tensors by a background thread instead of a
tf.FIFOQueue; with torch.distributed every rank reads a disjoint shard of each shuffled group (the reference
had one feeder for all towers); mulaw-quantize inputs stay class ids instead of materialising one-hot.

``SyntheticFeeder`` emits LJSpeech-shaped random tensors of the same layout (no dataset needed).
"""
import os
import queue
import threading

import numpy as np
import torch

from datasets import audio
from infolog import log
from wavenet_vocoder.util import is_mulaw_quantize, is_scalar_input

_batches_per_group = 64


def _interp(feats, in_range):
    """Rescale from in_range to [0, 1] (reference feeder.py:426-428)."""
    return (feats - in_range[0]) / (in_range[1] - in_range[0])


def _new_pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype, pin_memory=True)


def _ranks():
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank(), torch.distributed.get_world_size()
    return 0, 1


class Feeder(object):
    def __init__(self, coordinator, metadata_filename, base_dir, hparams, device=None):
        self._coord = coordinator
        self._hparams = hparams
        self._train_offset = 0
        self._test_offset = 0
        self._device = device
        self._rank, self._world = _ranks()
        self._rng = np.random.RandomState(hparams.wavenet_random_seed + 7919 * self._rank)      # crops: independent per rank
        self._order_rng = np.random.RandomState(hparams.wavenet_random_seed)                     # batch order: identical on every rank
        if hparams.symmetric_mels:
            self._spec_pad = -hparams.max_abs_value
        else:
            self._spec_pad = 0.
        self._base_dir = base_dir
        self._data_dir = os.path.dirname(metadata_filename)
        with open(metadata_filename, 'r', encoding='utf-8') as f:
            self._metadata = [line.strip().split('|') for line in f if line.strip()]
        from sklearn.model_selection import train_test_split
        indices = np.arange(len(self._metadata))
        test_size = hparams.wavenet_test_size if hparams.wavenet_test_size is not None else hparams.wavenet_test_batches * hparams.wavenet_batch_size
        train_indices, test_indices = train_test_split(indices, test_size=test_size, random_state=hparams.wavenet_data_random_state)
        # make the test set a multiple of the batch size
        len_test = (len(test_indices) // hparams.wavenet_batch_size) * hparams.wavenet_batch_size
        extra = test_indices[len_test:]
        test_indices = test_indices[:len_test]
        train_indices = np.concatenate([train_indices, extra])
        self._train_meta = [self._metadata[i] for i in train_indices]
        self._test_meta = [self._metadata[i] for i in test_indices]
        self._test_indices = [int(i) for i in test_indices]      # metadata rows of the test split (validation_batches)
        self.test_steps = len(self._test_meta) // hparams.wavenet_batch_size
        if hparams.wavenet_test_size is None:
            assert hparams.wavenet_test_batches == self.test_steps
        self.local_condition = hparams.cin_channels > 0
        self.global_condition = hparams.gin_channels > 0                     # reference feeder.py:353
        # feeder.py:267-268 (the reference asserts it while building the queue): fail at construction, not inside a thread
        if hparams.wavenet_batch_size % self._world != 0:
            raise ValueError('wavenet_batch_size ({}) must be divisible by the number of GPUs ({})'.format(hparams.wavenet_batch_size, self._world))
        self._train_q = queue.Queue(maxsize=8)
        self._eval_q = queue.Queue(maxsize=1)
        self._threads = []
        self._errors = {}
        self._pin_pool, self._pin_lock = {}, threading.Lock()
        self._len_cache = {}
        self._ahead, self._copy_stream = None, None

    # ------------------------------------------------------------------ threads
    def start_threads(self, session=None):
        # The producers are Python threads: while one holds the GIL in pure-Python code the training loop waits for the interpreter's
        # switch interval (5 ms by default -- half a training step) before it can enqueue the next kernels.  0.5 ms keeps the hand-off
        # latency far below the ~9 ms of device work the loop is ahead by (bench.py with_feeder: 10.6 -> see profiles/).
        import sys
        if sys.getswitchinterval() > 5e-4:
            sys.setswitchinterval(5e-4)
        for target in (self._enqueue_next_train_group, self._enqueue_next_test_group):
            t = threading.Thread(name='background', target=target, daemon=True)
            t.start()
            self._threads.append(t)

    def _should_stop(self):
        return self._coord is not None and self._coord.should_stop()

    def _producer(self, train, q):
        """Body of a background thread.  Any error (missing .npy, audio / mel length mismatch, '<no_g>' speaker column ...) travels
        through the queue BEHIND the batches that were already produced: next_*_batch re-raises it in the training loop when the
        loop reaches it.  The producer does not stop the coordinator itself -- the loop tests ``coord.should_stop()`` before every
        step and would leave silently, with up to 8 good batches still queued, a success message and (data parallel) the other
        ranks inside an all-reduce; the training loop owns the decision (train.py broadcasts the failure so every rank stops at
        the same step)."""
        try:
            while not self._should_stop():
                for batch in self._iter_group(train=train):
                    if self._put(q, self._pin(self._prepare_batch(batch), train)):
                        return
        except BaseException as e:          # noqa: BLE001 -- forwarded, not swallowed
            # The error belongs to THIS queue: its consumer reaches it behind the good batches (blocking put; gives up only when the
            # coordinator stops), and a consumer that finds the queue empty sees it in ``_errors``.  The other queue's consumer is
            # not told: a dead eval producer surfaces when rank 0 runs the eval step, and the training loop (train.py: ``agree``)
            # then stops every rank together.
            self._errors[id(q)] = e
            self._put(q, _FeederError(e))

    def _pin(self, batch, train=True):
        """numpy batch -> page-locked host tensors (in the producer thread, off the step's critical path): the H2D copies of
        next_*_batch are then truly asynchronous (``non_blocking`` from pageable memory is a synchronous staged copy).  The pinned
        buffers come from a small per-shape ring: ``tensor.pin_memory()`` allocates page-locked memory on every call (a driver call of
        ~1 ms per tensor: four per batch made the PRODUCER the bottleneck of a 10 ms step, bench.py ``with_feeder``)."""
        if not torch.cuda.is_available():
            return batch
        return self._pinned_batch(batch, train)

    _PIN_RING = 16      # slots per ring >= queue depth (8) + the batch being built + the three the consumer keeps referenced while their copies fly + slack

    def _pinned_batch(self, batch, train=True):
        """One ring SLOT holds the page-locked buffers of ONE whole batch (a buffer per tensor position).  The ring is keyed by the
        producer and by the (dtype, shape) of every tensor of the batch, so a slot is reused only PIN_RING batches later whatever the
        tensors look like.  (Round 4 keyed a ring per tensor shape: a mulaw-quantize batch, whose inputs and targets are the same
        int32 [B, T] array, took TWO buffers of one ring per batch, the ring covered 8 batches instead of 16, and with a full train
        queue batch k + 8 was staged into the input buffers of the still-queued batch k -- ADVICE round 4.)"""
        key = (bool(train),) + tuple(None if b is None else (b.dtype.str, b.shape) for b in batch)
        with self._pin_lock:
            ring = self._pin_pool.get(key)
            if ring is None:
                if len(self._pin_pool) >= 64:       # many distinct padded lengths (real data): drop the oldest shape's ring
                    self._pin_pool.pop(next(iter(self._pin_pool)))
                ring = self._pin_pool[key] = {'slots': [], 'next': 0}
            if len(ring['slots']) < self._PIN_RING:
                slot = [None if b is None else _new_pinned(torch.from_numpy(b).shape, torch.from_numpy(b).dtype) for b in batch]
                ring['slots'].append(slot)
            else:
                slot = ring['slots'][ring['next'] % self._PIN_RING]
            ring['next'] += 1
        for buf, b in zip(slot, batch):
            if b is not None:
                buf.copy_(torch.from_numpy(b))
        return tuple(slot)

    def _put(self, q, item):
        """Blocking put that gives up when the coordinator stops (returns True then)."""
        while True:
            try:
                q.put(item, timeout=0.5)
                return False
            except queue.Full:
                if self._should_stop():
                    return True

    def _enqueue_next_train_group(self):
        self._producer(True, self._train_q)

    def _enqueue_next_test_group(self):
        self._producer(False, self._eval_q)

    def _get(self, q):
        while True:
            try:
                item = q.get(timeout=1.0)
            except queue.Empty:
                err = self._errors.get(id(q))
                if err is not None:
                    raise RuntimeError('feeder thread failed: {!r}'.format(err)) from err
                continue
            if isinstance(item, _FeederError):
                raise RuntimeError('feeder thread failed: {!r}'.format(item.error)) from item.error
            return item

    def next_train_batch(self):
        """The next training batch as device tensors.  On a GPU the batch AFTER this one is already on its way: its H2D copies run on a
        copy stream while the current step computes (issued on the compute stream they cost the step ~0.1 ms of serialised SDMA launches
        at its very start), and the compute stream only waits for an event that has normally fired long ago.  A producer error met while
        prefetching is raised when THAT batch is asked for, so batches and errors keep their order."""
        dev = self._device or torch.device('cuda', torch.cuda.current_device())
        if dev.type != 'cuda':
            return self._to_device(self._get(self._train_q))
        if self._ahead is None:
            self._ahead = self._start_copy(self._get(self._train_q), dev)
        if isinstance(self._ahead, BaseException):
            err, self._ahead = self._ahead, None
            raise err
        tensors, ev = self._ahead
        self._ahead = None
        try:                                   # start the following batch if the producer already has it (never block for it here)
            item = self._train_q.get_nowait()
            if isinstance(item, _FeederError):
                self._ahead = RuntimeError('feeder thread failed: {!r}'.format(item.error))
                self._ahead.__cause__ = item.error
            else:
                self._ahead = self._start_copy(item, dev)
        except queue.Empty:
            pass
        cur = torch.cuda.current_stream(dev)
        cur.wait_event(ev)
        for t in tensors:
            if t is not None:
                t.record_stream(cur)            # allocated on the copy stream, used on the compute stream
        return tensors

    def _start_copy(self, batch, dev):
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        host = tuple(None if b is None else (b if torch.is_tensor(b) else torch.from_numpy(b)) for b in batch)
        self._inflight = (getattr(self, '_inflight', ()) + (host,))[-3:]      # pinned sources outlive their copies
        with torch.cuda.stream(self._copy_stream):
            tensors = tuple(None if b is None else b.to(dev, non_blocking=True) for b in host)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        return tensors, ev

    def next_eval_batch(self):
        return self._to_device(self._get(self._eval_q))

    def _to_device(self, batch):
        dev = self._device or torch.device('cuda', torch.cuda.current_device())
        host = tuple(None if b is None else (b if torch.is_tensor(b) else torch.from_numpy(b)) for b in batch)
        # double buffer: the pinned source of an in-flight copy must outlive it -- keep the last two batches referenced
        self._inflight = (getattr(self, '_inflight', ()) + (host,))[-2:]
        return tuple(None if b is None else b.to(dev, non_blocking=True) for b in host)

    # ------------------------------------------------------------------ examples
    def _next_group(self, train):
        """The batches (this rank's slices, arrays loaded) of the next group as a list."""
        return list(self._iter_group(train))

    def _iter_group(self, train):
        hp = self._hparams
        n = hp.wavenet_batch_size               # GLOBAL batch, divisible by the number of ranks (checked in __init__)
        # Every rank walks the SAME sequence of utterances (shared shuffles) but only reads the .npy HEADERS of the whole group
        # (length bucketing needs the lengths); the arrays themselves are loaded for this rank's slice of each batch only, so disk
        # and host work per step do not grow with the number of ranks.
        if train:
            metas = [self._next_meta(self._train_meta, True) for _ in range(n * _batches_per_group)]
            metas.sort(key=lambda m: m[1])                          # bucket by length (stable, like the reference's sort on len(x))
            batches = [metas[i:i + n] for i in range(0, len(metas), n)]
            # same order on every rank: at each step the ranks hold the disjoint slices of ONE length bucket (equal padding => equal step time)
            self._order_rng.shuffle(batches)
        else:
            metas = [self._next_meta(self._test_meta, False) for _ in range(len(self._test_meta))]
            batches = [metas[i:i + n] for i in range(0, len(metas), n)]
        per = n // self._world
        for b in batches:
            yield [self._load_example(m) for m, _ in b[self._rank * per:(self._rank + 1) * per]]

    def _next_meta(self, meta_list, train):
        """(metadata row, audio length) of the next utterance; the length comes from the .npy header (no data read)."""
        if train:
            if self._train_offset >= len(meta_list):
                self._train_offset = 0
                self._rng_shared_shuffle(meta_list)
            meta = meta_list[self._train_offset]; self._train_offset += 1
        else:
            if self._test_offset >= len(meta_list):
                self._test_offset = 0
            meta = meta_list[self._test_offset]; self._test_offset += 1
        return meta, self._length_of(meta[0])

    def _length_of(self, audio_path):
        """Samples of an utterance from its .npy header, read once per file (the bucketing of every 64-batch group needs 512 lengths:
        an mmap open per utterance and step was ~0.5 ms of GIL-holding work per step in the producer thread)."""
        n = self._len_cache.get(audio_path)
        if n is None:
            n = self._len_cache[audio_path] = int(np.load(self._resolve(audio_path), mmap_mode='r').shape[0])
        return n

    def _load_example(self, meta):
        hp = self._hparams
        mel_file = meta[2] if hp.train_with_GTA else meta[1]
        audio_file = meta[0]
        input_data = np.load(self._resolve(audio_file))
        local_feats = np.load(self._resolve(mel_file)) if self.local_condition else None
        if len(input_data) != len(local_feats) * audio.get_hop_size(hp):
            raise ValueError('audio / mel length mismatch in %s (%d samples vs %d frames x hop %d)'
                             % (audio_file, len(input_data), len(local_feats), audio.get_hop_size(hp)))
        g = None
        if self.global_condition:                                      # reference feeder.py:254-257: speaker id column of map.txt
            g = meta[3]
            if g == '<no_g>':
                raise RuntimeError('Please redo the wavenet preprocessing (or GTA synthesis) to assign global condition features!')
        return input_data, local_feats, g, len(input_data)

    def _rng_shared_shuffle(self, meta_list):
        # every rank shuffles identically so that the per-rank slices of a batch stay disjoint
        np.random.RandomState(self._hparams.wavenet_data_random_state + len(meta_list)).shuffle(meta_list)

    def _resolve(self, path):
        if os.path.isabs(path) or os.path.exists(path):
            return path
        for root in (self._base_dir, self._data_dir):
            cand = os.path.join(root, path)
            if os.path.exists(cand):
                return cand
        return path

    # ------------------------------------------------------------------ validation
    def validation_utterances(self, split='test'):
        """[(metadata row index, metadata row)] this rank scores, batch by batch, in validation_batches(split): metadata order; the utterances of
        every global batch of wavenet_batch_size are dealt to the ranks in contiguous slices (a short last batch leaves the last ranks short)."""
        if split not in ('test', 'all'):
            raise ValueError("validation split must be 'test' or 'all' (got %r)" % (split,))
        rows = sorted(self._test_indices) if split == 'test' else list(range(len(self._metadata)))
        n = self._hparams.wavenet_batch_size
        per = n // self._world
        out = []
        for i in range(0, len(rows), n):
            mine = rows[i:i + n][self._rank * per:(self._rank + 1) * per]
            if mine:
                out.append([(r, self._metadata[r]) for r in mine])
        return out

    def validation_batches(self, split='test'):
        """Generator over this rank's slice of the held-out split ('test'; 'all': the whole metadata file) as feeder-format device batches
        (inputs, targets, lengths, c, g): every utterance exactly once, in metadata order, the last batch possibly smaller.  Utterances
        longer than the time limit get a hop-aligned crop whose start is drawn from RandomState(wavenet_data_random_state + metadata row), so
        the split is the same at every validation of every run.  Files are read directly: the training / eval queues, offsets and random
        generators are not touched, so the sequence of training and eval batches does not depend on when (or whether) this runs."""
        hp = self._hparams
        dev = self._device or torch.device('cuda', torch.cuda.current_device())
        for group in self.validation_utterances(split):
            batch = [_limit_time([self._load_example(meta)], hp, np.random.RandomState(hp.wavenet_data_random_state + row))[0] for row, meta in group]
            yield tuple(None if b is None else torch.from_numpy(b).to(dev) for b in self._assemble_batch(batch))

    # ------------------------------------------------------------------ batch assembly
    def _prepare_batch(self, batch):
        hp = self._hparams
        batch = list(batch)
        self._rng.shuffle(batch)
        batch = _limit_time(batch, hp, self._rng)
        return self._assemble_batch(batch)

    def _assemble_batch(self, batch):
        """Padded numpy tensors of a list of (audio, mel, speaker, length) examples, in the order given."""
        hp = self._hparams
        input_lengths = np.asarray([len(x[0]) for x in batch], dtype=np.int32)
        max_t = int(input_lengths.max())
        hop = audio.get_hop_size(hp)
        if is_mulaw_quantize(hp.input_type):
            pad_v = 127
            x = np.stack([np.pad(b[0].astype(np.int32), (0, max_t - len(b[0])), constant_values=pad_v) for b in batch])
            inputs, targets = x, x                                     # class ids [B,T] (one-hot never materialised)
        else:
            x = np.stack([np.pad(b[0].astype(np.float32), (0, max_t - len(b[0]))) for b in batch])
            inputs = x[:, None, :]                                      # [B,1,T]
            targets = x[:, :, None]                                     # [B,T,1]
        max_c = max_t // hop
        T2 = (-hp.max_abs_value, hp.max_abs_value) if hp.symmetric_mels else (0., hp.max_abs_value)
        c = np.stack([np.pad(b[1].astype(np.float32), [(0, max_c - len(b[1])), (0, 0)], constant_values=self._spec_pad) for b in batch])
        if hp.clip_for_wavenet:
            c = np.clip(c, T2[0], T2[1])
        if hp.normalize_for_wavenet:
            c = _interp(c, T2)
        c = np.ascontiguousarray(c.transpose(0, 2, 1)).astype(np.float32)   # [B, num_mels, Tc]
        # global conditions: int32 speaker ids [B, 1] (reference feeder.py:342-349)
        g = np.array([b[2] for b in batch]).astype(np.int32).reshape(-1, 1) if self.global_condition else None
        return (np.ascontiguousarray(inputs), np.ascontiguousarray(targets), input_lengths, c, g)


class _FeederError(object):
    """Queue item that carries a producer thread's exception to the consumer."""

    def __init__(self, error):
        self.error = error


def _limit_time(batch, hparams, rng):
    """Hop-aligned random crop to max_time_steps (reference feeder.py:356-398)."""
    if hparams.max_time_sec is not None:
        max_time_steps = int(hparams.max_time_sec * hparams.sample_rate)
    elif hparams.max_time_steps is not None:
        max_time_steps = hparams.max_time_steps
    else:
        return batch
    hop = audio.get_hop_size(hparams)
    out = []
    for x, c, g, l in batch:
        max_steps = max_time_steps - max_time_steps % hop
        if len(x) > max_time_steps:          # (the reference compares with max_time_steps and draws start in [0, frames - max_frames), feeder.py:376-380)
            max_frames = max_steps // hop
            s = int(rng.randint(0, len(c) - max_frames))
            c = c[s:s + max_frames]
            x = x[s * hop:(s + max_frames) * hop]
        assert len(x) == len(c) * hop
        out.append((x, c, g, len(x)))
    return out


class SyntheticFeeder(object):
    """LJSpeech-shaped synthetic batches resident in HBM: smooth bounded waveform + U[0,1] mels."""

    def __init__(self, hparams, batch_size_per_rank, time_steps, device=None, n_distinct=4):
        self._hparams = hparams
        self._rank, self._world = _ranks()
        hop = audio.get_hop_size(hparams)
        self.T = int(time_steps) // hop * hop
        self.B = int(batch_size_per_rank)
        self.test_steps = 1
        dev = device or torch.device('cuda', torch.cuda.current_device())
        g = torch.Generator().manual_seed(hparams.wavenet_random_seed + 104729 * self._rank)
        self._batches = []
        for _ in range(n_distinct):
            t = torch.arange(self.T).float()
            f = torch.rand(self.B, 1, generator=g) * 320 + 80
            wav = (0.3 * torch.sin(2 * np.pi * f * t[None] / hparams.sample_rate) + 0.1 * torch.randn(self.B, self.T, generator=g)).clamp(-0.999, 0.999)
            c = torch.rand(self.B, hparams.cin_channels, self.T // hop, generator=g)
            lengths = torch.full((self.B,), self.T, dtype=torch.int32)
            if is_mulaw_quantize(hparams.input_type):
                from wavenet_vocoder.util import mulaw_quantize
                ids = torch.from_numpy(mulaw_quantize(wav.numpy())).int()
                x, y = ids, ids
            else:
                x, y = wav.view(self.B, 1, self.T), wav.view(self.B, self.T, 1)
            self._batches.append(tuple(v.contiguous().to(dev) for v in (x, y, lengths, c)) + (None,))
        self._i = 0

    def start_threads(self, session=None):
        pass

    def next_train_batch(self):
        b = self._batches[self._i % len(self._batches)]
        self._i += 1
        return b

    def next_eval_batch(self):
        return self._batches[0]

    def validation_batches(self, split='test'):
        """The held-out split of the synthetic data: the one eval batch (test_steps = 1), resident on the device."""
        yield self._batches[0]

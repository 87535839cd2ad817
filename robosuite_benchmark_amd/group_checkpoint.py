"""Checkpoints of a whole trainer group: every member's state in one directory, committed at once, with the replay buffers
stored in fixed chunks so that a save rewrites only the rows changed since the last one.

The solo format (checkpoint.py) writes each buffer whole at every save: at a 1e6-slot Lift buffer that is 369 MB per run
and epoch, 3.06 GB for Wipe, to record 2 500 new rows.  Here a buffer is `chunk_rows` storage rows per file; the manifest
maps each chunk of [0, size) to a file and its CRC32, and a chunk file is written only when rows in it changed since the
last committed save (dirty_chunks: from the buffer's monotonic rows-written counter and its ring cursor).  Unchanged
chunks stay in the files an earlier generation wrote and the new manifest points at them.

Layout under `<dir>`:
    gen-<n>/manifest.json           the group: per member its identity, trainer and buffer metadata and chunk map
    gen-<n>/m<i>.state.bin          member i: networks, Adam moments, trainer scalars, buffer generator key
    gen-<n>/m<i>.c<k>.bin           member i, buffer chunk k (written in generation n)
    latest                          names the newest complete generation; replaced atomically, last

Kill safety: a save writes only new files of a new generation directory (never one a committed manifest references),
fsyncs them and the manifest, then flips `latest`.  Files no manifest references any more are deleted only after the
flip.  A process killed at any point leaves either the old or the new generation complete, for every member at once."""
from __future__ import annotations

import hashlib
import json
import os
import time
import zlib
from collections import OrderedDict

import numpy as np

from .checkpoint import _fsync_dir, _generations, adopt_noise_seed

FORMAT = "robosuite_benchmark_amd.group_checkpoint/1"
DEFAULT_CHUNK_ROWS = 4096
HPARAMS = ("discount", "reward_scale", "policy_lr", "qf_lr", "soft_target_tau", "target_update_period",
           "use_automatic_entropy_tuning", "target_entropy", "noise_seed", "target_policy_noise",
           "target_policy_noise_clip", "policy_and_target_update_period")
BUFFER_KEYS = ("observations", "actions", "rewards", "next_observations", "terminals")


class GroupMismatchError(ValueError):
    """The live group is not the group the checkpoint holds (raised before any state is touched)."""


# ---- the dirty range ----------------------------------------------------------------------------------------------
def dirty_chunks(capacity, chunk_rows, size, top, rows_written, prev):
    """Chunk indices of [0, size) whose rows changed since the last committed save, sorted.

    prev: (rows_written, top, size) of the buffer at that save, or None (no save to build on: every chunk is dirty).
    The rows written since are the `rows_written - prev_rows_written` ring slots from prev_top on.  Every chunk is dirty
    when that count reaches the capacity, or when top / size are not where that many writes would have moved them
    (somebody moved the cursor)."""
    capacity, chunk_rows, size, top = int(capacity), int(chunk_rows), int(size), int(top)
    n_chunks = -(-size // chunk_rows)
    everything = list(range(n_chunks))
    if prev is None:
        return everything
    p_rw, p_top, p_size = (int(x) for x in prev)
    d = int(rows_written) - p_rw
    if d < 0 or d >= capacity:
        return everything
    if (p_top + d) % capacity != top or min(capacity, p_size + d) != size:
        return everything
    if d == 0:
        return []
    spans = [(p_top, min(p_top + d, capacity))]
    if p_top + d > capacity:                                  # the writes wrapped past the end of the ring
        spans.append((0, p_top + d - capacity))
    out = set()
    for a, b in spans:
        out.update(range(a // chunk_rows, (b - 1) // chunk_rows + 1))
    return sorted(k for k in out if k < n_chunks)


# ---- files --------------------------------------------------------------------------------------------------------
def _write(path, arrays):
    """One file holding the raw bytes of `arrays` back to back, fsynced.  Returns (bytes, CRC32)."""
    crc, n = 0, 0
    with open(path, "wb") as f:
        for a in arrays:
            mv = memoryview(np.ascontiguousarray(a)).cast("B")
            f.write(mv)
            crc, n = zlib.crc32(mv, crc), n + len(mv)
        f.flush()
        os.fsync(f.fileno())
    return n, crc & 0xFFFFFFFF


def _read(dirname, entry):
    """The bytes of a manifest entry {file, bytes, crc32}, checked."""
    path = os.path.join(dirname, entry["file"])
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) != entry["bytes"] or (zlib.crc32(blob) & 0xFFFFFFFF) != entry["crc32"]:
        raise ValueError(f"{path}: content does not match the group manifest (torn, damaged or foreign file)")
    return blob


def _split(blob, layout):
    """Arrays of `layout` [(name, dtype, shape)] from a blob _write made of them in that order."""
    out, off = OrderedDict(), 0
    for name, dtype, shape in layout:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out[name] = np.frombuffer(blob, dtype=dtype, count=int(np.prod(shape)), offset=off).reshape(shape).copy()
        off += n
    return out


def _chunk_layout(rows, O, A):
    return [("observations", "float32", (rows, O)), ("actions", "float32", (rows, A)), ("rewards", "float32", (rows, 1)),
            ("next_observations", "float32", (rows, O)), ("terminals", "uint8", (rows, 1))]


def _state_arrays(trainer, buffer):
    st = trainer.state_dict()
    arrays = OrderedDict()
    for net, flat in st["params"].items():
        arrays[f"params.{net}"] = np.ascontiguousarray(flat, np.float32)
    for net, (m, v) in st["opt"].items():
        arrays[f"adam_m.{net}"] = np.ascontiguousarray(m, np.float32)
        arrays[f"adam_v.{net}"] = np.ascontiguousarray(v, np.float32)
    arrays["trainer_scalars"] = np.ascontiguousarray(st["scalars"], np.float64)
    key, pos = buffer.rng_state()
    arrays["buffer.rng_key"] = np.ascontiguousarray(key, np.uint32)
    return arrays, int(pos)


def current_dir(dirname):
    """The newest complete generation under `dirname`, or None when nothing was ever committed there.  A `latest` that
    names a generation without a manifest is an error, not "no checkpoint" (a resuming group would start afresh and its
    first save would delete what is left)."""
    ptr = os.path.join(dirname, "latest")
    if not os.path.exists(ptr):
        return None
    with open(ptr) as f:
        sub = f.read().strip()
    cand = os.path.join(dirname, sub)
    if not sub or not os.path.exists(os.path.join(cand, "manifest.json")):
        raise FileNotFoundError(f"{dirname}: `latest` names '{sub}', which holds no manifest -- refusing to treat a "
                                "damaged group checkpoint as 'no checkpoint'")
    return cand


def checkpoint_exists(dirname):
    return os.path.isdir(dirname) and current_dir(dirname) is not None


def read_manifest(dirname):
    cdir = current_dir(dirname)
    if cdir is None:
        raise FileNotFoundError(f"{dirname}: no complete group checkpoint")
    with open(os.path.join(cdir, "manifest.json")) as f:
        man = json.load(f)
    if man.get("format") != FORMAT:
        raise ValueError(f"{cdir}: not a {FORMAT} checkpoint")
    return man


# ---- identity -----------------------------------------------------------------------------------------------------
def variant_hash(variant):
    """SHA-256 of the variant's JSON, without the epoch count (a resumed group may run to another epoch)."""
    v = json.loads(json.dumps(variant))
    v.get("algorithm_kwargs", {}).pop("num_epochs", None)
    return hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()


def member_identity(label, seed, variant, trainer):
    """What must agree between a live group member and its checkpointed counterpart."""
    return OrderedDict([
        ("label", str(label)), ("seed", int(seed)), ("algorithm", variant.get("algorithm", "SAC")),
        ("obs_dim", int(trainer.obs_dim)), ("action_dim", int(trainer.act_dim)), ("batch", int(trainer._batch)),
        ("policy_hidden", [int(h) for h in variant["policy_kwargs"]["hidden_sizes"]]),
        ("qf_hidden", [int(h) for h in variant["qf_kwargs"]["hidden_sizes"]]),
        ("variant_sha256", variant_hash(variant)),
        ("hparams", OrderedDict((k, getattr(trainer, k)) for k in HPARAMS if hasattr(trainer, k))),
    ])


def _check_identity(man, identities):
    saved = man["members"]
    for i in range(max(len(saved), len(identities))):
        if i >= len(saved) or i >= len(identities):
            who = identities[i]["label"] if i < len(identities) else saved[i]["identity"]["label"]
            raise GroupMismatchError(f"group member {i} ({who}): the group has {len(identities)} members, the "
                                     f"checkpoint {len(saved)}")
        live, want = json.loads(json.dumps(identities[i])), saved[i]["identity"]
        flat_live, flat_want = _flatten(live), _flatten(want)
        for k in list(flat_want) + [k for k in flat_live if k not in flat_want]:    # (the manifest's field order)
            if flat_live.get(k) != flat_want.get(k):
                raise GroupMismatchError(f"group member {i} ({live['label']}): {k} is {flat_live.get(k)!r} here, "
                                         f"{flat_want.get(k)!r} in the checkpoint")


def _flatten(ident):
    out = OrderedDict()
    for k, v in ident.items():
        if isinstance(v, dict):
            out.update((f"{k}.{h}", x) for h, x in v.items())
        else:
            out[k] = v
    return out


# ---- save / load --------------------------------------------------------------------------------------------------
class GroupCheckpoint:
    """Saves and loads the members of a trainer group under one directory.  Remembers, per member, the buffer counters
    and chunk map of the last committed save (or load), which the next save's dirty range is computed against."""

    def __init__(self, dirname, chunk_rows=DEFAULT_CHUNK_ROWS):
        if int(chunk_rows) <= 0:
            raise ValueError(f"chunk_rows must be positive (got {chunk_rows})")
        self.dirname, self.chunk_rows = dirname, int(chunk_rows)
        self._base = None              # per member: dict(prev=(rows_written, top, size), chunks=[...], offset=int)
        self.last_save = None          # dict(files=, bytes=, seconds=) of the last save

    def exists(self):
        return checkpoint_exists(self.dirname)

    def save(self, trainers, buffers, identities, extras):
        """Write one generation holding every member, then flip `latest` to it.  extras: JSON-serialisable dict per
        member (epoch, host generators ...)."""
        t0 = time.time()
        R = len(trainers)
        if not R == len(buffers) == len(identities) == len(extras):
            raise ValueError("save needs one trainer, buffer, identity and extra per member")
        base = self._base if self._base is not None and len(self._base) == R else [None] * R
        os.makedirs(self.dirname, exist_ok=True)
        gens = _generations(self.dirname)
        sub = f"gen-{(gens[-1] + 1) if gens else 0}"
        gdir = os.path.join(self.dirname, sub)
        os.makedirs(gdir)
        man = dict(format=FORMAT, chunk_rows=self.chunk_rows, members=[])
        new_base, n_files, n_bytes = [], 0, 0
        for i, (tr, buf, ident, extra) in enumerate(zip(trainers, buffers, identities, extras)):
            if getattr(tr, "_h", None) is None:
                raise RuntimeError(f"group member {i} owns no device state yet")
            arrays, rng_pos = _state_arrays(tr, buf)
            name = f"m{i}.state.bin"
            nb, crc = _write(os.path.join(gdir, name), arrays.values())
            n_files, n_bytes = n_files + 1, n_bytes + nb
            state = dict(file=f"{sub}/{name}", bytes=nb, crc32=crc,
                         layout=[(k, str(a.dtype), list(a.shape)) for k, a in arrays.items()])
            cap, O, A = buf._max_replay_buffer_size, buf._observation_dim, buf._action_dim
            size, top = int(buf.num_steps_can_sample()), int(buf.top())
            b = base[i]
            offset = b["offset"] if b else 0
            rw = int(buf.rows_written()) + offset
            dirty = set(dirty_chunks(cap, self.chunk_rows, size, top, rw, b["prev"] if b else None))
            chunks = []
            for k in range(-(-size // self.chunk_rows)):
                r0 = k * self.chunk_rows
                rows = min(self.chunk_rows, size - r0)
                old = b["chunks"][k] if b and k < len(b["chunks"]) else None
                if k in dirty or old is None or old["rows"] != rows:
                    cname = f"m{i}.c{k}.bin"
                    nb, crc = _write(os.path.join(gdir, cname), buf.read_rows(r0, rows))
                    old = dict(file=f"{sub}/{cname}", rows=rows, bytes=nb, crc32=crc)
                    n_files, n_bytes = n_files + 1, n_bytes + nb
                chunks.append(old)
            man["members"].append(dict(
                identity=ident, extra=extra, state=state,
                trainer=dict(num_train_steps=int(tr._num_train_steps), batch_size=int(tr._batch)),
                buffer=dict(capacity=int(cap), obs_dim=int(O), action_dim=int(A), top=top, size=size, rows_written=rw,
                            rng_pos=rng_pos, chunks=chunks)))
            new_base.append(dict(prev=(rw, top, size), chunks=chunks, offset=offset))
        with open(os.path.join(gdir, "manifest.json"), "w") as f:
            json.dump(man, f, indent=1)
            f.flush()
            os.fsync(f.fileno())
        _fsync_dir(gdir)
        tmp = os.path.join(self.dirname, "latest.tmp")
        with open(tmp, "w") as f:
            f.write(sub + "\n")
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, os.path.join(self.dirname, "latest"))         # the commit point
        _fsync_dir(self.dirname)
        self._base = new_base
        self._collect(man, sub)
        self.last_save = dict(files=n_files, bytes=n_bytes, seconds=time.time() - t0)
        return man

    def _collect(self, man, sub):
        """After the flip: delete every file of the other generations that `man` does not reference (older saves, torn
        ones), and the generation directories left empty."""
        keep = {m["state"]["file"] for m in man["members"]} | {c["file"] for m in man["members"] for c in m["buffer"]["chunks"]}
        for g in _generations(self.dirname):
            gname = f"gen-{g}"
            if gname == sub:
                continue
            gdir = os.path.join(self.dirname, gname)
            for name in os.listdir(gdir):
                if f"{gname}/{name}" not in keep:
                    try:
                        os.remove(os.path.join(gdir, name))
                    except OSError:
                        pass
            try:
                os.rmdir(gdir)                                          # (only succeeds once it is empty)
            except OSError:
                pass

    def load(self, trainers, buffers, identities):
        """Restore every member from the newest generation; returns the members' extras.  The live group is checked
        against the manifest and every file's CRC is verified, for all members, before any state is touched."""
        man = read_manifest(self.dirname)
        _check_identity(man, identities)
        if int(man["chunk_rows"]) != self.chunk_rows:
            self.chunk_rows = int(man["chunk_rows"])                  # the layout on disk decides
        states = [self._verify(man, i, m, buffers[i]) for i, m in enumerate(man["members"])]
        base = []
        for tr, buf, m, st in zip(trainers, buffers, man["members"], states):
            base.append(_restore(self.dirname, tr, buf, m, st))
        self._base = base
        return [m["extra"] for m in man["members"]]

    def _verify(self, man, i, m, buf):
        bm = m["buffer"]
        if (bm["capacity"], bm["obs_dim"], bm["action_dim"]) != (
                buf._max_replay_buffer_size, buf._observation_dim, buf._action_dim):
            raise GroupMismatchError(f"group member {i} ({m['identity']['label']}): replay buffer (capacity, obs_dim, "
                                     f"action_dim) is {(buf._max_replay_buffer_size, buf._observation_dim, buf._action_dim)}"
                                     f" here, {(bm['capacity'], bm['obs_dim'], bm['action_dim'])} in the checkpoint")
        state = _split(_read(self.dirname, m["state"]), m["state"]["layout"])
        for c in bm["chunks"]:
            _read(self.dirname, c)
        return state


def _restore(dirname, trainer, buf, m, arrays, noise_seed=None):
    """One member from its verified state arrays and chunk files: the trainer's state, then the buffer as
    EnvReplayBuffer.load_state_dict restores one (rows in storage order, cursor, generator).  noise_seed: the saved
    member's, for a trainer that was not checked against the member's identity (load_group_member)."""
    nets = [k[len("params."):] for k in arrays if k.startswith("params.")]
    st = dict(params={n: arrays[f"params.{n}"] for n in nets},
              opt={n: (arrays[f"adam_m.{n}"], arrays[f"adam_v.{n}"]) for n in nets if f"adam_m.{n}" in arrays},
              scalars=arrays["trainer_scalars"])
    adopt_noise_seed(trainer, noise_seed, int(m["trainer"]["batch_size"]))
    trainer.load_state_dict(st)
    trainer._num_train_steps = int(m["trainer"]["num_train_steps"])
    bm = m["buffer"]
    O, A = bm["obs_dim"], bm["action_dim"]
    buf.set_cursor(0, 0)
    for c in bm["chunks"]:
        blob = _read(dirname, c)
        rows = _split(blob, _chunk_layout(c["rows"], O, A))
        buf.add_block(*(rows[k] for k in BUFFER_KEYS))
    buf.set_cursor(bm["top"], bm["size"])
    buf.set_rng_state(arrays["buffer.rng_key"], bm["rng_pos"])
    live = int(buf.rows_written())
    return dict(prev=(int(bm["rows_written"]), int(bm["top"]), int(bm["size"])), chunks=bm["chunks"],
                offset=int(bm["rows_written"]) - live)


def load_group_member(dirname, index, trainer, buffer):
    """Member `index` of the group checkpoint under `dirname` into an ordinary trainer and replay buffer (a run can then
    go on solo, on the member's noise stream: checkpoint.adopt_noise_seed).  Returns the member's extra (epoch, seed, host
    generators, collector totals)."""
    man = read_manifest(dirname)
    if not 0 <= int(index) < len(man["members"]):
        raise IndexError(f"{dirname}: the group has {len(man['members'])} members, no member {index}")
    m = man["members"][int(index)]
    ident = m["identity"]
    if (ident["obs_dim"], ident["action_dim"]) != (trainer.obs_dim, trainer.act_dim):
        raise GroupMismatchError(f"group member {index} ({ident['label']}): dims ({trainer.obs_dim},{trainer.act_dim}) "
                                 f"here, ({ident['obs_dim']},{ident['action_dim']}) in the checkpoint")
    st = GroupCheckpoint(dirname, man["chunk_rows"])._verify(man, int(index), m, buffer)
    _restore(dirname, trainer, buffer, m, st, noise_seed=ident.get("hparams", {}).get("noise_seed"))
    return m["extra"]

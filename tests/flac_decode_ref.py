"""A FLAC decoder in plain Python and numpy, written from RFC 9639 and from nothing else: the bar for csrc/flac.hip.

decode(data) parses "fLaC" and the metadata blocks (STREAMINFO is read, any other block is skipped), then every frame: header with
the UTF-8-like coded number, block-size and sample-rate codes and their tail fields, CRC-8; the subframes (CONSTANT, VERBATIM, FIXED,
LPC; wasted bits; both Rice methods, with their escape codes); the stereo decorrelation (left/side, side/right, mid/side); padding and
CRC-16.  It insists on what the RFC asks of a stream: reserved bits zero, both CRCs right, frames (or samples, in a variable-blocksize
stream) numbered consecutively from zero, every block but the last of STREAMINFO's size, the block sizes summing to STREAMINFO's
total, each frame's size inside STREAMINFO's bounds, no bytes left over.  Anything else raises FlacError.

Returns (pcm, info, frames): pcm (samples, channels) -- int16 for 16 bits a sample, int32 otherwise --, info = STREAMINFO's fields,
frames = one record per frame: number, blocksize and its code, header bytes, assignment ("independent", "left/side", "side/right", "mid/side"), size in bytes,
offset in the file, and per subframe its type, order, partition order, Rice method, number of escaped partitions, wasted bits and
size in bits."""
import shutil
import subprocess

import numpy as np


class FlacError(ValueError):
    pass


def _crc_table(poly, width):
    top, mask, table = 1 << (width - 1), (1 << width) - 1, []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _CRC8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xffff) ^ _CRC16[(c >> 8) ^ b]
    return c


class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos, self.end = data, pos * 8, len(data) * 8

    def read(self, n):
        if n == 0:
            return 0
        p = self.pos
        if p + n > self.end:
            raise FlacError("the stream ends inside a field")
        self.pos = p + n
        b = (p + n + 7) >> 3
        return (int.from_bytes(self.data[p >> 3:b], "big") >> (b * 8 - p - n)) & ((1 << n) - 1)

    def signed(self, n):
        v = self.read(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        """Number of zero bits in front of the next one bit; the one bit is consumed."""
        q = 0
        while True:
            p = self.pos
            if p >= self.end:
                raise FlacError("the stream ends inside a unary code")
            n = min(32, self.end - p)
            b = (p + n + 7) >> 3
            w = (int.from_bytes(self.data[p >> 3:b], "big") >> (b * 8 - p - n)) & ((1 << n) - 1)
            if w:
                z = n - w.bit_length()
                self.pos = p + z + 1
                return q + z
            q += n
            self.pos = p + n


_BLOCK = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_DEPTH = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_ASSIGN = {8: "left/side", 9: "side/right", 10: "mid/side"}


def _residual(br, blocksize, order, rec):
    method = br.read(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    porder = br.read(4)
    parts = 1 << porder
    if blocksize % parts or (order and (blocksize >> porder) <= order):
        raise FlacError("partition order %d does not fit block size %d, predictor order %d" % (porder, blocksize, order))
    rec.update(partition_order=porder, rice_method=method, escapes=0)
    out = []
    for q in range(parts):
        count = (blocksize >> porder) - (order if q == 0 else 0)
        k = br.read(pbits)
        if k == esc:
            nb = br.read(5)
            rec["escapes"] += 1
            out.extend(br.signed(nb) for _ in range(count))
        else:
            unary, read = br.unary, br.read
            for _ in range(count):
                z = (unary() << k) | read(k)
                out.append((z >> 1) ^ -(z & 1))
    return out


def _subframe(br, blocksize, bps):
    if br.read(1):
        raise FlacError("subframe padding bit set")
    kind = br.read(6)
    start = br.pos - 7
    wasted = 0
    if br.read(1):
        wasted = br.unary() + 1
        bps -= wasted
    rec = dict(type=None, order=0, partition_order=None, rice_method=None, escapes=0, wasted=wasted)
    if kind == 0:
        rec["type"] = "CONSTANT"
        s = np.full(blocksize, br.signed(bps), dtype=np.int64)
    elif kind == 1:
        rec["type"] = "VERBATIM"
        s = np.array([br.signed(bps) for _ in range(blocksize)], dtype=np.int64)
    elif 8 <= kind <= 12:
        order = kind - 8
        rec.update(type="FIXED", order=order)
        if order > blocksize:
            raise FlacError("FIXED order above the block size")
        warm = np.array([br.signed(bps) for _ in range(order)], dtype=np.int64)
        cur = np.array(_residual(br, blocksize, order, rec), dtype=np.int64)
        for lvl in range(order - 1, -1, -1):           # the order-lvl differences from sample `order` on: a running sum from the warm-up's
            cur = np.diff(warm, lvl)[-1] + np.cumsum(cur)
        s = np.concatenate([warm, cur])
    elif kind >= 32:
        order = kind - 31
        rec.update(type="LPC", order=order)
        if order > blocksize:
            raise FlacError("LPC order above the block size")
        s = [br.signed(bps) for _ in range(order)]
        prec = br.read(4) + 1
        if prec == 16:
            raise FlacError("reserved coefficient precision")
        shift = br.signed(5)
        if shift < 0:
            raise FlacError("negative predictor shift")
        coef = [br.signed(prec) for _ in range(order)]
        rec.update(precision=prec, shift=shift, coefficients=list(coef))
        coef_r = coef[::-1]                              # coefficient j multiplies sample i - 1 - j
        for i, r in enumerate(_residual(br, blocksize, order, rec)):
            s.append(r + (sum(c * x for c, x in zip(coef_r, s[i:i + order])) >> shift))
        s = np.array(s, dtype=np.int64)
    else:
        raise FlacError("reserved subframe type %d" % kind)
    rec["bits"] = br.pos - start
    return s << wasted, rec


def _frame(data, pos, info):
    br = _Bits(data, pos)
    if br.read(15) != 0x7ffc:
        raise FlacError("no frame sync (or its reserved bit set) at byte %d" % pos)
    variable = br.read(1)
    bcode, rcode, assign, dcode = br.read(4), br.read(4), br.read(4), br.read(3)
    if br.read(1):
        raise FlacError("reserved bit set in a frame header")
    first = br.read(8)                                   # the coded number: 0xxxxxxx, or 110xxxxx 10xxxxxx, ... up to 7 bytes
    extra = 0
    while first & (0x80 >> extra):
        extra += 1
    if extra == 1 or extra > 7:
        raise FlacError("malformed coded number")
    number = first & (0x7f >> extra) if extra else first
    for _ in range(max(extra - 1, 0)):
        b = br.read(8)
        if b >> 6 != 2:
            raise FlacError("malformed coded number")
        number = (number << 6) | (b & 0x3f)
    if bcode == 0:
        raise FlacError("reserved block size code")
    blocksize = br.read(8) + 1 if bcode == 6 else br.read(16) + 1 if bcode == 7 else _BLOCK[bcode]
    if rcode == 15:
        raise FlacError("forbidden sample rate code")
    rate = (info["sample_rate"] if rcode == 0 else br.read(8) * 1000 if rcode == 12 else br.read(16) if rcode == 13
            else br.read(16) * 10 if rcode == 14 else _RATE[rcode])
    if dcode == 3:
        raise FlacError("reserved sample size code")
    bps = info["bits_per_sample"] if dcode == 0 else _DEPTH[dcode]
    if crc8(data[pos:br.pos >> 3]) != br.read(8):
        raise FlacError("frame %d: CRC-8 mismatch" % number)
    header_bytes = (br.pos >> 3) - pos
    if assign > 10:
        raise FlacError("reserved channel assignment")
    channels = assign + 1 if assign < 8 else 2
    if (rate, bps, channels) != (info["sample_rate"], info["bits_per_sample"], info["channels"]):
        raise FlacError("frame %d disagrees with STREAMINFO" % number)
    side = {8: 1, 9: 0, 10: 1}.get(assign)
    subs, recs = [], []
    for c in range(channels):
        s, rec = _subframe(br, blocksize, bps + (1 if c == side else 0))
        subs.append(s)
        recs.append(rec)
    if assign == 8:
        subs = [subs[0], subs[0] - subs[1]]
    elif assign == 9:
        subs = [subs[0] + subs[1], subs[1]]
    elif assign == 10:
        mid = (subs[0] << 1) | (subs[1] & 1)
        subs = [(mid + subs[1]) >> 1, (mid - subs[1]) >> 1]
    pad = -br.pos % 8
    if br.read(pad):
        raise FlacError("frame %d: padding bits set" % number)
    end = br.pos >> 3
    if crc16(data[pos:end]) != br.read(16):
        raise FlacError("frame %d: CRC-16 mismatch" % number)
    rec = dict(number=number, variable=variable, blocksize=blocksize, assignment=_ASSIGN.get(assign, "independent"), size=end + 2 - pos,
               offset=pos, header_bytes=header_bytes, blocksize_code=bcode, subframes=recs)
    return np.stack(subs, 1), rec, end + 2


def decode(data):
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, info, last = 4, None, False
    while not last:
        if pos + 4 > len(data):
            raise FlacError("the stream ends inside the metadata")
        last, kind, length = data[pos] >> 7, data[pos] & 0x7f, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + length]
        if len(body) != length or kind == 127:
            raise FlacError("bad metadata block")
        if info is None:
            if kind != 0 or length != 34:
                raise FlacError("the first metadata block is not STREAMINFO")
            v = int.from_bytes(body[10:18], "big")
            info = dict(min_blocksize=int.from_bytes(body[0:2], "big"), max_blocksize=int.from_bytes(body[2:4], "big"),
                        min_framesize=int.from_bytes(body[4:7], "big"), max_framesize=int.from_bytes(body[7:10], "big"),
                        sample_rate=v >> 44, channels=((v >> 41) & 7) + 1, bits_per_sample=((v >> 36) & 31) + 1,
                        total_samples=v & ((1 << 36) - 1), md5=body[18:34], metadata_blocks=0)
        elif kind == 0:
            raise FlacError("a second STREAMINFO block")
        info["metadata_blocks"] += 1
        pos += 4 + length
    if info["min_blocksize"] < 16 or info["max_blocksize"] < info["min_blocksize"] or info["sample_rate"] == 0:
        raise FlacError("STREAMINFO out of range")
    info["audio_offset"] = pos
    chunks, frames, samples = [], [], 0
    while pos < len(data):
        pcm, rec, pos = _frame(data, pos, info)
        if rec["variable"] != (frames[0]["variable"] if frames else rec["variable"]):
            raise FlacError("blocking strategy changes inside the stream")
        if rec["number"] != (samples if rec["variable"] else len(frames)):
            raise FlacError("frame %d is numbered %d" % (len(frames), rec["number"]))
        if frames and frames[-1]["blocksize"] != info["max_blocksize"] and not rec["variable"]:
            raise FlacError("a short block that is not the last")
        if rec["blocksize"] > info["max_blocksize"]:
            raise FlacError("frame %d: block size above STREAMINFO's" % rec["number"])
        if info["min_framesize"] and not info["min_framesize"] <= rec["size"] <= info["max_framesize"]:
            raise FlacError("frame %d: size %d outside STREAMINFO's bounds" % (rec["number"], rec["size"]))
        samples += rec["blocksize"]
        chunks.append(pcm)
        frames.append(rec)
    if frames and info["min_framesize"]:
        sizes = [r["size"] for r in frames]
        if (min(sizes), max(sizes)) != (info["min_framesize"], info["max_framesize"]):
            raise FlacError("STREAMINFO's frame sizes are not the stream's")
    if samples != info["total_samples"]:
        raise FlacError("the blocks hold %d samples, STREAMINFO says %d" % (samples, info["total_samples"]))
    pcm = np.concatenate(chunks) if chunks else np.zeros((0, info["channels"]), dtype=np.int64)
    lim = 1 << (info["bits_per_sample"] - 1)
    if pcm.size and (pcm.min() < -lim or pcm.max() >= lim):
        raise FlacError("a decoded sample does not fit %d bits" % info["bits_per_sample"])
    return pcm.astype(np.int16 if info["bits_per_sample"] == 16 else np.int32), info, frames


def other_decoder():
    """An independent decoder found on this machine, or None: 'soundfile' (libsndfile) or the 'flac' command-line tool."""
    try:
        import soundfile  # noqa: F401
        return "soundfile"
    except Exception:
        return "flac" if shutil.which("flac") else None


def decode_with_other(data, tmp_path):
    """(samples, channels) int16 from whichever other decoder other_decoder() found."""
    path = str(tmp_path / "pin.flac")
    with open(path, "wb") as f:
        f.write(bytes(data))
    if other_decoder() == "soundfile":
        import soundfile
        pcm, _ = soundfile.read(path, dtype="int16", always_2d=True)
        return pcm
    channels = decode(data)[1]["channels"]
    raw = subprocess.run([shutil.which("flac"), "-d", "-s", "-c", "--force-raw-format", "--endian=little", "--sign=signed", path],
                         capture_output=True, check=True).stdout
    return np.frombuffer(raw, dtype="<i2").reshape(-1, channels)

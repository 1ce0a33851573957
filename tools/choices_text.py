"""The settled launch choices (vr_export_choices) as committed text: profiles/launch_choices.json <-> profiles/launch_choices.bin.

The blob bench.py imports (profiles/launch_choices.bin) is binary and is not kept in git; what is committed is its exact field-by-field
restatement in profiles/launch_choices.json, and __graft_entry__.build() writes the binary back from it, byte for byte.  After an
evidence pass has measured a new blob (tools/round_evidence.sh, phase 0), turn it into the committed text with

    python tools/choices_text.py encode [profiles/launch_choices.bin] [profiles/launch_choices.json]

Layout (launch_tuner.h: ChoiceHeader / ChoiceRecord, little-endian): header "VRCHOICE", u32 version, u32 count, u64 build id,
char[64] device model; then per entry u64 key, i32 ncand, i32 settled candidate, i32 heuristic candidate, i32 cand[8], 4 bytes padding.
"""
from __future__ import annotations

import json
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "profiles" / "launch_choices.bin"
TEXT = ROOT / "profiles" / "launch_choices.json"
_HEADER, _RECORD = "<8sIIQ64s", "<Qiii8i4x"


def encode(blob: bytes) -> dict:
    magic, version, count, build_id, device = struct.unpack_from(_HEADER, blob, 0)
    if magic != b"VRCHOICE" or len(blob) != struct.calcsize(_HEADER) + count * struct.calcsize(_RECORD):
        raise ValueError("not a vr_export_choices blob")
    entries = []
    for i in range(count):
        key, ncand, settled, heur, *cand = struct.unpack_from(_RECORD, blob, struct.calcsize(_HEADER) + i * struct.calcsize(_RECORD))
        entries.append({"key": f"0x{key:016x}", "ncand": ncand, "settled": settled, "heur": heur, "cand": cand})
    out = {"format": "vr_export_choices blob, version 1 (tools/choices_text.py)", "version": version, "build_id": f"0x{build_id:016x}",
           "device": device.split(b"\0")[0].decode(), "entries": entries}
    if decode(out) != blob:
        raise ValueError("the blob does not restate losslessly (non-zero padding)")
    return out


def decode(doc: dict) -> bytes:
    entries = doc["entries"]
    device = doc["device"].encode()
    if len(device) >= 64:
        raise ValueError("device string too long")
    b = struct.pack(_HEADER, b"VRCHOICE", int(doc["version"]), len(entries), int(doc["build_id"], 16), device)
    for e in entries:
        cand = list(e["cand"])
        if len(cand) != 8:
            raise ValueError("cand holds 8 slots")
        b += struct.pack(_RECORD, int(e["key"], 16), int(e["ncand"]), int(e["settled"]), int(e["heur"]), *cand)
    return b


def dumps(doc: dict) -> str:
    """the committed text: the header fields, then one entry per line"""
    head = {k: v for k, v in doc.items() if k != "entries"}
    lines = ",\n".join("  " + json.dumps(e) for e in doc["entries"])
    return json.dumps(head, indent=1)[:-2] + ',\n "entries": [\n' + lines + "\n ]\n}\n"


def write_blob(text: Path = TEXT, blob: Path = BIN) -> bool:
    """profiles/launch_choices.bin from the committed text (False: no committed text)"""
    if not text.exists():
        return False
    data = decode(json.loads(text.read_text()))
    if not blob.exists() or blob.read_bytes() != data:
        blob.write_bytes(data)
    return True


def main(argv):
    if len(argv) >= 2 and argv[1] == "encode":
        src = Path(argv[2]) if len(argv) > 2 else BIN
        dst = Path(argv[3]) if len(argv) > 3 else TEXT
        dst.write_text(dumps(encode(src.read_bytes())))
    elif len(argv) >= 2 and argv[1] == "decode":
        write_blob(Path(argv[2]) if len(argv) > 2 else TEXT, Path(argv[3]) if len(argv) > 3 else BIN)
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

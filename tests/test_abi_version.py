"""The ABI version the header defines (and uwspr_get_info reports) is the last entry of its own changelog, and the
entry points of that entry are declared and bound."""
import os
import re


def _header(G):
    return open(os.path.join(os.path.dirname(G.native.CSRC), "..", "include", "uwspr_hip.h")).read()


def test_abi_version_matches_its_changelog(G):
    hdr = _header(G)
    m = re.search(r"#define UWSPR_ABI_VERSION (\d+)\s*/\*(.*?)\*/", hdr, re.S)
    assert m, "UWSPR_ABI_VERSION with its changelog comment"
    entries = [int(v) for v in re.findall(r"(?:^|\s)(\d+):", m.group(2))]
    assert entries == sorted(entries) and entries[-1] == int(m.group(1)) == 6, (m.group(1), entries)


def test_audio_stream_entry_points_are_declared_and_bound(G):
    hdr = _header(G)
    for name in ("uwspr_stream_push_audio", "uwspr_pipe_push_audio"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in G.native.ABI_SYMBOLS
    assert re.search(r"UWSPR_AUDIO_F32 = 0, UWSPR_AUDIO_S16 = 1", hdr)
    assert (G.native.AUDIO_F32, G.native.AUDIO_S16) == (0, 1)

"""Device and pinned host memory has one kind of owner in the native sources: DeviceArray / PinnedArray of
osg_device_buffer.h.  An object that lives as long as a solver holds its buffers through them, so nothing keeps a list
of what to free.

(a) The runtime's allocation calls appear in that header only.
(b) struct osg_cfr, struct MmdState, struct osg_ctx and struct osg_batch declare no raw `T* d_... = nullptr` /
    `T* h_... = nullptr` member."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_spiel_amd", "csrc")
OWNER_HEADER = "osg_device_buffer.h"
ALLOCATION_CALL = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\(")
OWNING_STRUCTS = ("osg_cfr", "MmdState", "osg_ctx", "osg_batch")
# `int32_t *d_a = nullptr, *d_b = nullptr;`, `double* h_out = nullptr;`, `double* d_x[2] = {nullptr, nullptr};`
RAW_MEMBER = re.compile(r"\*\s*(?:const\s+)?([dh]_\w+)\s*(?:\[\w*\]\s*)?=\s*\{?\s*nullptr")


def _sources():
    sources = [p for ext in ("hip", "h", "cc", "cpp") for p in glob.glob(os.path.join(CSRC, "**", f"*.{ext}"), recursive=True)]
    assert sources
    return sorted(sources)


def _struct_body(text, name):
    """The text between `struct NAME {` and its closing brace."""
    m = re.search(r"^struct %s \{" % re.escape(name), text, re.M)
    if not m:
        return None
    depth, at = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[at], 0)
        at += 1
    return text[m.end():at - 1]


def test_allocation_calls_only_in_the_owner_header():
    found = []
    for path in _sources():
        if os.path.basename(path) == OWNER_HEADER:
            continue
        with open(path) as f:
            for no, line in enumerate(f.read().splitlines(), 1):
                if ALLOCATION_CALL.search(line):
                    found.append(f"{os.path.relpath(path, ROOT)}:{no}: {line.strip()}")
    assert not found, "allocation calls outside osg_device_buffer.h (hold the buffer in a DeviceArray / PinnedArray):\n" + "\n".join(found)
    # the header does make them
    with open(os.path.join(CSRC, OWNER_HEADER)) as f:
        assert {m.group(1) for m in ALLOCATION_CALL.finditer(f.read())} == {"hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree"}


def test_owning_structs_hold_no_raw_device_or_pinned_members():
    texts = {}
    for path in _sources():
        with open(path) as f:
            texts[path] = f.read()
    for name in OWNING_STRUCTS:
        bodies = [(p, _struct_body(t, name)) for p, t in texts.items()]
        bodies = [(p, b) for p, b in bodies if b is not None]
        assert len(bodies) == 1, f"struct {name} defined in {[os.path.relpath(p, ROOT) for p, _ in bodies]}"
        path, body = bodies[0]
        raw = RAW_MEMBER.findall(body)
        assert not raw, f"struct {name} ({os.path.relpath(path, ROOT)}) holds raw members: {raw}"


def test_the_raw_member_pattern_sees_what_it_forbids():
    for line in ("  double* d_disc = nullptr;", "  int32_t *d_a = nullptr, *d_b = nullptr;", "  unsigned int* h_sub_err = nullptr;",
                 "  double* d_spare_delta[2] = {nullptr, nullptr};", "          *d_mem_off = nullptr, *d_mem = nullptr;", "  void* d_words = nullptr;",
                 "  unsigned long long* d_illegal = nullptr;  // device counter of illegal applies"):
        assert RAW_MEMBER.search(line), line
    for line in ("  DeviceArray<double> d_tables;", "  osg_ctx* ctx = nullptr;", "  const char* last_kernel = \"\";",
                 "  std::unique_ptr<MmdState> mmd;"):
        assert not RAW_MEMBER.search(line), line

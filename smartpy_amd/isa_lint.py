"""Checks of the BUILT library's gfx950 code that the sources alone cannot give: the pieces of the kernels whose
correctness rests on where hipcc's assembler put an instruction.

  pair blocks   smart_forcing_scan writes byte offsets ("code words") into the blocks of the streaming step loops
                (smart_fast_arms.h: SMART_A_PAIRS_STRETCH, SMART_A_GAP_STREAM, SMART_A_EVERY_STREAM); a block that
                outgrew its room or changed its place would send a computed jump into the middle of another
  hand-over     the publish / wait sequences of the time-sliced kernels (smart_device.h: publish_slice,
                wait_for_slice) as MI355X_MICROARCH.md prescribes them -- hipcc drops a wait it can prove unnecessary
  rows          the DPP chains of the row form of the literal step (smart_literal_lanes.h): inline asm is opaque to
                hipcc's hazard recogniser, so the two wait states gfx950 wants between a vector write of a register
                and a DPP read of it are the source's own business

smartpy_amd.build runs all three on every library it links (lint_and_record): the verdict on the pair blocks goes into
the file itself (stamp_library) and the whole outcome next to it (<lib>.lint.json, with `hipcc --version` and the
library's sha256).  smartpy_amd._lib reads that record when it loads the library: a library whose pair blocks failed
the lint -- or that is not the one the lint looked at, e.g. rebuilt by another hipcc on another box -- runs the threaded
chunks (SMART_PAIR_BLOCKS=0: the same arithmetic without computed jumps) behind a warning; a library whose hand-over
or row chains failed is refused.  The tests (tests/test_pair_blocks_isa.py, test_handover_isa.py, test_lanes_isa.py)
call the same functions.

llvm-objdump of the ROCm toolchain is needed; without it check_library() says so and nothing is claimed.
"""
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess
import tempfile


def _find_objdump():
    """llvm-objdump of the ROCm toolchain: $ROCM_PATH, the usual place, or whatever the PATH holds"""
    roots = [os.environ.get('ROCM_PATH'), os.environ.get('ROCM_HOME'), '/opt/rocm']
    for root in roots:
        if root:
            exe = os.path.join(root, 'lib', 'llvm', 'bin', 'llvm-objdump')
            if os.path.exists(exe):
                return exe
    return shutil.which('llvm-objdump') or '/opt/rocm/lib/llvm/bin/llvm-objdump'


OBJDUMP = _find_objdump()

# smart_capi.hip: the exported `char smart_lint_stamp[40]`.  The verdict on the pair blocks is written INTO the library
# file there: a caller of the C ABI, who reads no record next to it, gets the computed jumps only from code that was looked at
STAMP_SYMBOL, STAMP_SIZE = b'smart_lint_stamp', 40
STAMP_UNCHECKED = b'SMART_LINT_STAMP=unchecked'
STAMP_PAIRS_OK = b'SMART_LINT_STAMP=pairs-ok\0'          # (same length: the one written over the other)


def _stamp_offset(path):
    """Where in the file smart_lint_stamp lies, by the dynamic symbol table of an ELF64 little-endian library (None for
    any other file, and without the symbol).  Its text is NOT searched for: the same text may stand elsewhere in the
    image, as a constant of the code that compares it."""
    with open(path, 'rb') as fh:
        blob = fh.read()
    try:
        if blob[:6] != b'\x7fELF\x02\x01':
            return None
        shoff, = struct.unpack_from('<Q', blob, 0x28)
        shentsize, shnum = struct.unpack_from('<HH', blob, 0x3a)
        # (name, type, flags, addr, offset, size, link, info, addralign, entsize) of every section
        sections = [struct.unpack_from('<IIQQQQIIQQ', blob, shoff + i * shentsize) for i in range(shnum)]
        for _, _, _, _, offset, size, link, _, _, entsize in [sec for sec in sections if sec[1] == 11]:     # SHT_DYNSYM
            strings = sections[link][4]
            for sym in range(offset, offset + size, entsize):
                name, _, _, shndx, value, length = struct.unpack_from('<IBBHQQ', blob, sym)
                if blob[strings + name:blob.index(b'\0', strings + name)] == STAMP_SYMBOL and length == STAMP_SIZE:
                    at = value - sections[shndx][3] + sections[shndx][4]
                    return at if 0 <= at <= len(blob) - STAMP_SIZE else None
    except (struct.error, ValueError, IndexError):
        pass                        # (a truncated or doctored file)
    return None


def library_stamp(path):
    """'pairs-ok' | 'unchecked' | None (no stamp in the file)"""
    at = _stamp_offset(path)
    if at is None:
        return None
    with open(path, 'rb') as fh:
        fh.seek(at)
        text = fh.read(STAMP_SIZE).split(b'\0')[0]
    return {STAMP_PAIRS_OK.rstrip(b'\0'): 'pairs-ok', STAMP_UNCHECKED: 'unchecked'}.get(text)


def stamp_library(path, pairs_ok):
    """Write the verdict on the pair blocks into the library file, whatever stood there.  -> was the stamp found?"""
    at = _stamp_offset(path)
    if at is None:
        return False
    with open(path, 'r+b') as fh:
        fh.seek(at)
        fh.write((STAMP_PAIRS_OK if pairs_ok else STAMP_UNCHECKED).ljust(STAMP_SIZE, b'\0'))
    return True


HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, 'csrc', 'libsmart_amd.so')
FP64 = ('v_fma_f64', 'v_fmac_f64', 'v_add_f64', 'v_mul_f64', 'v_min_f64', 'v_max_f64', 'v_ldexp_f64')

SLICED = ['smart_fast_intervals_exits', 'smart_fast_intervals', 'smart_fast_intervals_states', 'smart_fast_runs_exits',
          'smart_fast_runs', 'smart_fast_runs_states', 'smart_fast_steps', 'smart_fast_steps_states',
          'smart_fast_steps_raw', 'smart_fast_intervals_raw', 'smart_fast_steps_every']
PAIRED = ['smart_fast_steps', 'smart_fast_steps_raw', 'smart_fast_steps_states']
ROWS = ['smart_fast_illcond', 'smart_ensemble_literal_rows']

KINDS = 'CDR'          # smart_device.h: step_kind -- 0 calm, 1 dry, 2 rain
FIRST = {'C': 'v_cmp_lt_f64', 'D': 'v_mul_f64', 'R': 'v_mov_b64'}      # how the three arms begin
PAIRS = [k0 + k1 for k0 in KINDS for k1 in KINDS]       # a pair of steps: the nine patterns, in the order of their blocks


class LintError(Exception):
    pass


def _need(cond, message):
    if not cond:
        raise LintError(message)


def classify(op):
    base = op.replace('_e32', '').replace('_e64', '')
    if base in FP64:
        return 'fp64'
    if base.startswith('v_cmp'):
        return 'vcmp'
    if base.startswith(('v_mov', 'v_cndmask', 'v_accvgpr')):
        return 'vmov'
    if base.startswith(('v_readlane', 'v_writelane', 'v_readfirstlane')):
        return 'lane'
    if base.startswith('v_'):
        return 'valu'
    if base.startswith(('s_branch', 's_cbranch')):
        return 'branch'
    if base.startswith(('s_load', 's_store', 's_buffer_load', 's_dcache')):
        return 'smem'
    if base.startswith(('global_', 'buffer_', 'flat_', 'scratch_', 'ds_')):
        return 'vmem'
    if base.startswith(('s_waitcnt', 's_nop', 's_sleep', 's_endpgm', 's_barrier', 's_code_end', 's_setprio', 's_trap')):
        return 'other'
    if base.startswith('s_'):
        return 'salu'
    return 'other'


def parse(start, body):
    insts = []
    for line in body.split('\n'):
        m = re.match(r'\s+(\S+)\s*(.*?)\s*//\s*([0-9A-F]+):\s*[0-9A-F ]+(?:<[^+>]+\+0x([0-9a-f]+)>)?\s*$', line)
        if not m:
            continue
        op, args, addr, off = m.group(1), m.group(2), int(m.group(3), 16), m.group(4)
        target = start + int(off, 16) if off is not None and classify(op) == 'branch' else None
        insts.append({'addr': addr, 'op': op, 'args': args, 'cls': classify(op), 'target': target})
    return insts


class Disassembly(object):
    """The gfx950 code objects bundled in a shared library, disassembled once (llvm-objdump --offloading writes them
    next to its input: done on a copy in a scratch directory); kernel(name) -> its instructions."""

    def __init__(self, lib=LIB):
        if not os.path.exists(OBJDUMP):
            raise LintError('llvm-objdump of the ROCm toolchain not found (%s)' % OBJDUMP)
        self.lib = lib
        tmp = tempfile.mkdtemp(prefix='smart_isa_')
        try:
            copy = os.path.join(tmp, os.path.basename(lib))
            shutil.copy(lib, copy)
            subprocess.run([OBJDUMP, '--offloading', copy], check=True, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL)
            self.texts = [subprocess.run([OBJDUMP, '-d', os.path.join(tmp, f)], check=True, capture_output=True,
                                         text=True).stdout for f in sorted(os.listdir(tmp)) if 'gfx950' in f]
        finally:
            shutil.rmtree(tmp)
        self._cache = {}

    def raw(self, kernel):
        for text in self.texts:
            m = re.search(r'^([0-9a-f]+) <(_ZN5smart\d+%s[A-Z][^>]*)>:\n(.*?)(?=^\S|\Z)' % re.escape(kernel), text,
                          re.M | re.S)
            if m:
                return int(m.group(1), 16), m.group(2), m.group(3)
        raise LintError('kernel %s not found in %s' % (kernel, self.lib))

    def kernel(self, name):
        if name not in self._cache:
            start, _, body = self.raw(name)
            insts = parse(start, body)
            for a, b in zip(insts, insts[1:]):
                a['size'] = b['addr'] - a['addr']
            if insts:
                insts[-1]['size'] = 4
            self._cache[name] = insts
        return self._cache[name]


def _disassembly(lib_or_dis):
    return lib_or_dis if isinstance(lib_or_dis, Disassembly) else Disassembly(lib_or_dis or LIB)


def _define(name):
    text = open(os.path.join(HERE, 'csrc', 'smart_device.h')).read()
    return int(re.search(r'#define %s (\d+)' % name, text).group(1))


def fast_kernel_table():
    """{name: is it one of a time-sliced family} as the library itself lists its fast kernels (SMART_FAST_KERNELS in
    smart_fast_entry.h)"""
    text = open(os.path.join(HERE, 'csrc', 'smart_fast_entry.h')).read()
    return {name: sliced == 'true' for name, sliced in re.findall(r'^\s*X\(k\w+, (smart_fast_\w+), \d, (true|false), ', text, re.M)}


# ---- pair blocks ----------------------------------------------------------------------------------------------------
def _block_base(insts, i):
    return insts[i]['addr'] + 4 + int(insts[i + 1]['args'].split(',')[-1], 0)


def _entries(insts):
    return [i for i, x in enumerate(insts) if x['op'] == 's_getpc_b64' and 's[78:79]' in x['args']]


def _walk_blocks(insts, i, stride, names, count, what='block'):
    """The blocks of the streaming loop behind the entry at instruction i: block n, `stride` bytes behind block n - 1, runs
    steps of the kinds names[n].  Each must be what the code words assume: it starts on an instruction -- a block that
    begins with the rain arm is entered 4 bytes in (pair_code adds 4), so an s_nop stands on its boundary --, with the
    first instruction of its first arm, and its main path reaches the computed jump inside its room.  Yields, per block,
    (n, names[n], index of its s_setpc_b64, {prefix: instructions of the main path that begin with it} for `count`)."""
    at = {x['addr']: k for k, x in enumerate(insts)}
    base = _block_base(insts, i)
    _need(base % 64 == 0, '%s 0 at %#x is not on a 64-byte line' % (what, base))
    for n, kinds in enumerate(names):
        where, b = '%s %d (%s)' % (what, n, kinds), base + n * stride
        _need(b in at, '%s does not start on an instruction' % where)
        k = at[b]
        if kinds[0] == 'R':
            _need(insts[k]['op'] == 's_nop' and insts[k]['size'] == 4, '%s: no s_nop on the boundary' % where)
            k += 1
        _need(insts[k]['op'].startswith(FIRST[kinds[0]]), '%s begins with %s' % (where, insts[k]['op']))
        seen = dict.fromkeys(count, 0)
        while insts[k]['op'] != 's_setpc_b64':
            _need(insts[k]['addr'] < b + stride, '%s outgrew its %d bytes' % (where, stride))
            for prefix in count:
                seen[prefix] += insts[k]['op'].startswith(prefix)
            k += 1
        yield n, kinds, k, seen


def _check_pair_instance(insts, i, stride):
    """SMART_A_PAIRS_STRETCH: 36 pair blocks (buffer 0: first pair, second pair; buffer 1: first, second; nine patterns
    each), then 4 of a whole chunk (four calm, four dry steps; per buffer)"""
    _need(insts[i + 1]['op'] == 's_add_u32' and insts[i + 1]['args'].startswith('s78, s78,'), 'entry without its s_add_u32')
    base = _block_base(insts, i)
    # the entry (the second form has two: a stretch may start in either buffer) ends with the jump to the first block,
    # nothing falls into the blocks
    j, last = i, insts[i]
    while insts[j]['addr'] < base:
        last = insts[j]
        j += 1
    while last['op'] == 's_nop':
        j -= 1
        last = insts[j - 1]
    _need(last['op'] == 's_setpc_b64', 'the entry falls into block 0 (%s in front of it)' % last['op'])
    for n, kinds, k, seen in _walk_blocks(insts, i, stride, PAIRS * 4 + ['CCCC', 'DDDD'] * 2, ('s_load_dwordx16',)):
        _need(insts[k]['args'].strip() == 's[76:77]', 'block %d (%s): jump through %s' % (n, kinds, insts[k]['args']))
        # a first pair's tail requests nothing; a second pair's, and a whole chunk's, the chunk after next
        _need(seen['s_load_dwordx16'] == (n // 9 % 2 if n < 36 else 1),
              'block %d (%s) requests %d chunks' % (n, kinds, seen['s_load_dwordx16']))
        # what follows the jump (out-of-line cascades) stays inside the block's room and ends with a branch back
        room = base + (n + 1) * stride
        end = insts[k]['addr'] + 4
        m = k + 1
        while m < len(insts) and insts[m]['addr'] < room:
            if insts[m]['op'].startswith(('v_', 's_branch', 's_cbranch')):
                end = insts[m]['addr'] + insts[m]['size']
            m += 1
        _need(end <= room or n == 39, 'block %d (%s): its out-of-line code outgrew the room' % (n, kinds))


def _check_gap_stream(insts, i, stride):
    """SMART_A_GAP_STREAM: 54 blocks, 2 buffers x 3 variants (no report in the pair / behind its first arm / behind its
    second) x 9 patterns; every main path requests one pair and holds the report's row-pointer move exactly where its
    variant says"""
    for n, kinds, _, seen in _walk_blocks(insts, i, stride, PAIRS * 6, ('s_load_dwordx16', 'v_lshl_add_u64'), 'stream block'):
        loads, reports = seen['s_load_dwordx16'], seen['v_lshl_add_u64']
        _need(loads == 1 and reports == (n % 27 >= 9), 'stream block %d (%s): %d loads, %d reports' % (n, kinds, loads, reports))


def lint_pair_blocks(lib=None, kernel=None):
    """Every block of the streaming step loops lies where smart_forcing_scan's code words point.  Raises LintError."""
    dis = _disassembly(lib)
    for name in ([kernel] if kernel else PAIRED):
        split = name.endswith('_states')    # the models with the final state vector: larger blocks, no stream of records
        stride = _define('SMART_PS_STRIDE' if split else 'SMART_P_STRIDE')
        _need(stride % 64 == 0, 'stride %d is no multiple of 64' % stride)
        insts = dis.kernel(name)
        entries = _entries(insts)
        # the stream of records (SMART_A_GAP_STREAM) loads ONE code word per pair, the pair blocks two per chunk
        pairs = [i for i in entries if not any(x['op'] == 's_load_dword' for x in insts[i:i + 12])]
        _need(len(pairs) == 2, '%s: %d instances of the stretch asm (two: even / any number of chunks)' % (name, len(pairs)))
        try:
            for i in pairs:
                _check_pair_instance(insts, i, stride)
            streams = [i for i in entries if i not in pairs]
            _need(len(streams) == (0 if split else 1), '%s: %d streams of records' % (name, len(streams)))
            if streams:
                _check_gap_stream(insts, streams[0], _define('SMART_E_STRIDE'))
        except LintError as e:
            raise LintError('%s: %s' % (name, e))
    if kernel is None or kernel == 'smart_fast_steps_every':
        lint_every_stream(dis)


def lint_every_stream(lib=None):
    """SMART_A_EVERY_STREAM (a report every step): four instances in smart_fast_steps_every (matrix stored or not,
    observations or not), each 2 x 9 blocks SMART_E_STRIDE bytes apart; every block's main path -- arm, report, arm,
    report, loop control -- requests exactly one pair of steps, and the two instances that store the matrix store it in
    every arm"""
    dis = _disassembly(lib)
    stride = _define('SMART_E_STRIDE')
    _need(stride % 64 == 0, 'stride %d is no multiple of 64' % stride)
    insts = dis.kernel('smart_fast_steps_every')
    entries = _entries(insts)
    try:
        _need(len(entries) == 4, '%d instances of the stream (four)' % len(entries))
        stores = []
        for i in entries:
            stores.append(0)
            for n, kinds, _, seen in _walk_blocks(insts, i, stride, PAIRS * 2, ('s_load_dwordx16', 'global_store_dwordx2')):
                _need(seen['s_load_dwordx16'] == 1, 'block %d (%s) requests %d pairs' % (n, kinds, seen['s_load_dwordx16']))
                stores[-1] += seen['global_store_dwordx2']
        _need(sorted(stores) == [0, 0, 36, 36], 'stores per instance %r' % (stores,))
    except LintError as e:
        raise LintError('smart_fast_steps_every: %s' % e)


# ---- hand-over ------------------------------------------------------------------------------------------------------
def _is_wait_vm0(x):
    return x['op'] == 's_waitcnt' and 'vmcnt(0)' in x['args']


def _is_payload_access(x):
    """a vector-memory access that is neither a flag access (sc1) nor an atomic"""
    return x['cls'] == 'vmem' and x['op'].startswith(('global_load', 'global_store', 'flat_load', 'flat_store',
                                                      'buffer_load', 'buffer_store')) and 'sc1' not in x['args']


def lint_handover(lib=None, kernel=None):
    """  producer   s_waitcnt vmcnt(0) -> buffer_wbl2 sc1 -> s_waitcnt vmcnt(0) -> global_store_dword ... sc1 (the flag)
         consumer   global_load_dword ... sc1 (the poll) -> s_waitcnt vmcnt(0) -> buffer_inv sc1 -> plain loads
    at every publish and every wait of every sliced kernel; and no kernel that publishes is missing from SLICED."""
    dis = _disassembly(lib)
    for name in ([kernel] if kernel else SLICED):
        insts = dis.kernel(name)
        releases = [i for i, x in enumerate(insts) if x['op'] == 'buffer_wbl2']
        polls = [i for i, x in enumerate(insts) if x['op'] == 'global_load_dword' and 'sc1' in x['args']]
        # a sliced body publishes in two places (a slice that ran; a slice that gave up and poisons its chain) and waits
        # in one; the compiler may duplicate either, it may not lose one
        _need(len(releases) >= 2 and len(polls) >= 1, '%s: %d publishes, %d waits' % (name, len(releases), len(polls)))
        for i in releases:
            _need('sc1' in insts[i]['args'], '%s: buffer_wbl2 without sc1 (agent scope)' % name)
            # straight-line from the write-back to the flag store: a wait for it, and nothing that signals before the wait
            j = i + 1
            waited = False
            while j < len(insts) and not (insts[j]['op'].startswith(('global_store', 'global_atomic')) and
                                          ('sc1' in insts[j]['args'] or insts[j]['op'].startswith('global_atomic'))):
                waited = waited or _is_wait_vm0(insts[j])
                _need(waited or insts[j]['cls'] not in ('vmem', 'branch'),
                      '%s: %s %s between buffer_wbl2 and its wait' % (name, insts[j]['op'], insts[j]['args']))
                j += 1
            _need(j < len(insts) and waited, '%s: no s_waitcnt vmcnt(0) between buffer_wbl2 and the flag store' % name)
            _need(insts[j]['op'] == 'global_store_dword' and 'sc1' in insts[j]['args'], '%s: the flag store is %s' % (name, insts[j]['op']))
            # ... and ahead of the write-back the wave's own payload stores have been waited for
            k = i - 1
            while k >= 0 and insts[k]['cls'] not in ('vmem', 'branch'):
                if _is_wait_vm0(insts[k]):
                    break
                k -= 1
            _need(k >= 0 and _is_wait_vm0(insts[k]), '%s: payload stores not drained ahead of buffer_wbl2' % name)
        for i in polls:
            # behind the poll (in address order: the exit of the poll loop lies behind it) the L1 invalidate comes before
            # the first plain load of the hand-over; its own wait stands directly in front of it
            j = i + 1
            while j < len(insts) and insts[j]['op'] != 'buffer_inv':
                _need(not _is_payload_access(insts[j]),
                      '%s: %s %s between the poll and buffer_inv' % (name, insts[j]['op'], insts[j]['args']))
                j += 1
            _need(j < len(insts) and 'sc1' in insts[j]['args'], '%s: no buffer_inv sc1 behind the poll' % name)
            _need(_is_wait_vm0(insts[j - 1]), '%s: buffer_inv without its wait' % name)
    if kernel is None:
        table = fast_kernel_table()
        _need(len(table) >= 12 and set(SLICED) == {n for n, sliced in table.items() if sliced},
              'the list of sliced kernels does not match the library\'s')
        for name in table:
            publishes = any(x['op'] == 'buffer_wbl2' for x in dis.kernel(name))
            _need(publishes == (name in SLICED), '%s publishes but is not linted as a sliced kernel (or the reverse)' % name)


# ---- the row form's DPP chains ----------------------------------------------------------------------------------------
def _regs(token):
    """v[4:5] -> {4, 5}; v7 -> {7}; anything else -> empty (-v[2:3] and |v1| included)"""
    m = re.match(r'^[-|]*v\[(\d+):(\d+)\]\|?$', token)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'^[-|]*v(\d+)\|?$', token)
    return {int(m.group(1))} if m else set()


def _dest_regs(x):
    """the vector registers a vector instruction writes (its first operand), none for compares and stores"""
    if not x['op'].startswith('v_') or x['cls'] == 'vcmp' or x['op'].startswith(('v_readlane', 'v_readfirstlane')):
        return set()
    first = x['args'].split(',')[0].strip()
    return _regs(first)


def lint_rows(lib=None, kernel=None):
    """Every DPP instruction of the row-form kernels: no vector instruction within the two wait states in front of it
    writes the register it reads through DPP (src0; s_nop N counts N + 1), and no v_cmpx (a vector write of EXEC)
    within five.  Counted over the preceding instructions in address order AND, at the target of a branch, over the
    instructions in front of every branch that leads there.  Also: the kernels do hold the chains (>= 100 DPP
    instructions each), so that an empty check cannot pass."""
    dis = _disassembly(lib)
    for name in ([kernel] if kernel else ROWS):
        insts = dis.kernel(name)
        at = {x['addr']: i for i, x in enumerate(insts)}
        sources = {}
        for i, x in enumerate(insts):
            if x['cls'] == 'branch' and x['target'] in at:
                sources.setdefault(at[x['target']], []).append(i)

        def writers_before(i, need):
            """(instruction, wait states between it and instruction i) for every instruction that can execute within
            `need` wait states ahead of i, along fall-through and branches"""
            found, stack, seen = [], [(i, 0)], set()
            while stack:
                j, dist = stack.pop()
                for src in sources.get(j, []):          # arriving by a branch: the branch itself is one wait state
                    if (src, dist + 1) not in seen and dist + 1 <= need:
                        seen.add((src, dist + 1))
                        stack.append((src, dist + 1))
                k = j - 1
                if k < 0 or insts[k]['op'] in ('s_endpgm', 's_branch', 's_setpc_b64'):
                    continue                              # nothing falls through from there
                y = insts[k]
                if dist < need:
                    found.append((y, dist))
                step = 1 + (int(y['args'].strip() or 0) if y['op'] == 's_nop' else 0)
                if dist + step < need and (k, dist + step) not in seen:
                    seen.add((k, dist + step))
                    stack.append((k, dist + step))
            return found

        n_dpp = 0
        for i, x in enumerate(insts):
            if 'row_newbcast' not in x['args'] and 'row_shl' not in x['args'] and 'row_shr' not in x['args']:
                continue
            n_dpp += 1
            ops = [t.strip() for t in x['args'].split(' row_')[0].split(',')]
            src0 = _regs(ops[1]) if len(ops) > 1 else set()
            _need(src0, '%s: cannot read the DPP operand of %s %s' % (name, x['op'], x['args']))
            for y, dist in writers_before(i, 2):
                _need(not (_dest_regs(y) & src0),
                      '%s: %s %s at %#x reads through DPP what %s %s wrote %d wait state(s) earlier (two are needed)'
                      % (name, x['op'], x['args'], x['addr'], y['op'], y['args'], dist))
            for y, dist in writers_before(i, 5):
                _need(not y['op'].startswith('v_cmpx'),
                      '%s: %s at %#x follows a vector write of EXEC (%s) by %d wait states (five are needed)'
                      % (name, x['op'], x['addr'], y['op'], dist))
        _need(n_dpp >= 100, '%s holds %d DPP instructions: the row form is not in it' % (name, n_dpp))


# ---- the library as a whole -----------------------------------------------------------------------------------------
def sha256_of(path):
    h = hashlib.sha256()
    with open(path, 'rb') as fh:
        for chunk in iter(lambda: fh.read(1 << 20), b''):
            h.update(chunk)
    return h.hexdigest()


def hipcc_version():
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    try:
        out = subprocess.run([exe, '--version'], capture_output=True, text=True, timeout=60).stdout
        return ' | '.join(ln.strip() for ln in out.splitlines() if ln.strip())[:400]
    except Exception as e:      # noqa: BLE001
        return 'unknown (%s)' % e


def check_library(lib=LIB):
    """Run the three lints on `lib`.  -> {'sha256', 'hipcc', 'checked', 'pair_blocks', 'handover', 'rows', 'problems'}:
    each of the three True / False (None when llvm-objdump is missing: nothing checked)."""
    report = {'library': os.path.basename(lib), 'sha256': sha256_of(lib), 'hipcc': hipcc_version(), 'checked': False,
              'pair_blocks': None, 'handover': None, 'rows': None, 'problems': []}
    try:
        dis = Disassembly(lib)
    except LintError as e:
        report['problems'].append(str(e))
        return report
    report['checked'] = True
    for key, fn in (('pair_blocks', lint_pair_blocks), ('handover', lint_handover), ('rows', lint_rows)):
        try:
            fn(dis)
            report[key] = True
        except LintError as e:
            report[key] = False
            report['problems'].append('%s: %s' % (key, e))
    return report


def sidecar_path(lib=LIB):
    return lib + '.lint.json'


def write_sidecar(report, lib=LIB):
    tmp = '%s.%d.tmp' % (sidecar_path(lib), os.getpid())
    with open(tmp, 'w') as fh:
        json.dump(report, fh, indent=1)
        fh.write('\n')
    os.replace(tmp, sidecar_path(lib))


def read_sidecar(lib=LIB):
    try:
        with open(sidecar_path(lib)) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return None


def record_state(lib=LIB):
    """Is there a record next to the library that counts for it?  'none' | 'other-build' (written for another file: the
    library was rebuilt by something else, or the record travelled alone) | 'this-build'"""
    rep = read_sidecar(lib)
    if rep is None:
        return 'none'
    return 'this-build' if rep.get('sha256') == sha256_of(lib) else 'other-build'


def verdict_of(report, sha256):
    """What smartpy_amd._lib does with a library of that sha256, given a report of check_library
    -> (ok_to_load, pair_blocks_ok, reason).  A report counts only for the very file it was made for."""
    if report.get('sha256') != sha256:
        return True, False, 'the lint record next to the library was written for another build of it'
    if not report.get('checked'):
        return True, False, 'the library was built without llvm-objdump at hand: its code was not looked at'
    if report.get('handover') is False or report.get('rows') is False:
        return False, False, '; '.join(report.get('problems', []))
    if not report.get('pair_blocks'):
        return True, False, '; '.join(report.get('problems', []))
    return True, True, ''


def verdict_for(lib=LIB):
    """verdict_of the record next to the library"""
    rep = read_sidecar(lib)
    if rep is None:
        return True, False, 'no lint record next to the library (%s): not built by smartpy_amd.build' % os.path.basename(sidecar_path(lib))
    return verdict_of(rep, sha256_of(lib))


def lint_and_record(path, record_for=None, stamp=False, check=check_library):
    """Look at the library at `path`, stamp it if asked (the build does, on a file nobody has mapped yet; the loader never
    rewrites the file it is about to map) and leave the report, for the file as it now is, next to `record_for`: the
    name the library is installed under, `path` by default.  -> the report (all there is of it in a read-only tree)."""
    report = check(path)
    if stamp:
        stamp_library(path, bool(report['pair_blocks']))
        report['sha256'] = sha256_of(path)
    report['stamp'] = library_stamp(path)
    try:
        write_sidecar(report, record_for or path)
    except OSError:
        pass
    return report


if __name__ == '__main__':
    import sys
    rep = check_library(sys.argv[1] if len(sys.argv) > 1 else LIB)
    print(json.dumps(rep, indent=1))
    sys.exit(0 if rep['checked'] and not rep['problems'] else 1)

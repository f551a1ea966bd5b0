"""tools/stamp_config.py's placement report (host-only): the decoding of the hardware-id words a stamped diagnostic build records per
(workgroup slot, role) — HW_ID bits 5:4 SIMD, 11:8 CU, 12 shader array, 15:13 shader engine; XCC_ID bits 3:0; the wave's index in its
workgroup in the upper half of the second word — and the busy / idle split of a role between the tick's barrier and the role barrier."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("stamp_config", os.path.join(ROOT, "tools", "stamp_config.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _buffer(sc, slots, simd_of, t_tick=1000, busy=(200, 150, 80, 40), t_role=1300):
    h = [0] * sc.STAMP_WORDS
    base = sc.SLOTS * 4 * 16
    for s in range(slots):
        for role in range(4):
            row = 64 * s + 16 * role
            h[row + 1], h[row + 13], h[row + 2], h[row + 3] = 900, t_tick, t_tick + busy[role], t_role
            hw = (simd_of(s, role) << 4) | (5 << 8) | (1 << 12) | (3 << 13) | 7   # wave slot 7, CU 5, SH 1, SE 3
            h[base + (4 * s + role) * 2] = hw
            h[base + (4 * s + role) * 2 + 1] = 6 | (((role - s) & 3) << 32)      # XCC 6; role = (wave + slot) & 3
    return h


def test_placement_decodes_ids_and_splits_busy_from_idle():
    sc = _tool()
    assert sc.STAMP_WORDS == 16 * 4 * 16 + 16 * 4 * 2
    where = sc.Placement()
    for _ in range(3):
        where.add(_buffer(sc, 4, lambda s, role: (role + s) & 3), 4, 64)
    assert list(where.cu) == [(6, 3, 1, 5)]
    c = where.cu[(6, 3, 1, 5)]
    assert c["n"] == 12
    assert c["simd"] == [[3, 3, 3, 3]] * 4                      # every role on every SIMD once per launch
    assert [round(b / c["n"], 6) for b in c["busy"]] == [2.0, 1.5, 0.8, 0.4]      # 100 ticks per us
    assert [round(i / c["n"], 6) for i in c["idle"]] == [1.0, 1.5, 2.2, 2.6]
    assert where.same_simd == [0, 0, 0, 0, 12]                  # four waves, four SIMDs
    assert where.role_simd == [[3, 3, 3, 3]] * 4
    # the wave's index in its workgroup is (role - slot) & 3 here, its SIMD (role + slot) & 3: wave w sits on SIMD (w + 2 slot) & 3
    assert where.wave_simd == [[6, 0, 6, 0], [0, 6, 0, 6], [6, 0, 6, 0], [0, 6, 0, 6]]
    assert where.tiles[3][0] == 192


def test_placement_sees_pinned_roles():
    sc = _tool()
    where = sc.Placement()
    where.add(_buffer(sc, 16, lambda s, role: role), 16, 1)
    assert where.role_simd == [[16, 0, 0, 0], [0, 16, 0, 0], [0, 0, 16, 0], [0, 0, 0, 16]]
    where.report()

"""csrc/nwt_map.hpp, the one memory map of the structured Newton mode and the QP-based SQP step, compiled for the host
(tests/drivers/nwt_map_drv.cpp) over a table of shapes -- one and several groups, two-sided on and off, with and without free outputs, QP on
and off, 128 / 256 / 512 lanes, odd nC and ncnln -- against the three formulas it replaced, restated here (they are the specification):
the workspace doubles of plan_solve.cpp's nwt_doubles, the LDS bytes and the reduction scratch of ntg_make_layout, and the offsets sqp_kernel
computed for itself.  The areas of each region follow one another without overlap and end at the totals."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
IN = "nC ncnln P ngrp ng hb tw ja jb nfo ngf cg nt qp".split()
OUT = "Kb B U lamq c jwg a JU total npad ncq ylen lena lenb yb panel npan yf ylenf qa qpd slots red act bytes red_doubles flag".split()
NWT_PANEL, NWT_STAGE, QP_MAXCG, QP_RED = 416, 216, 6, 128


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nwt_map") / "nwt_map_drv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(HERE, "drivers", "nwt_map_drv.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = [dict(zip(IN + OUT, map(int, line.split()))) for line in out.splitlines()]
    assert len(rows) == 8 * 3 * 2 and all(len(r) == len(IN + OUT) for r in rows)
    return rows


def qp_maxa(ngrp, nt):
    return 32 if ngrp == 1 and nt >= 256 else 16


def qp_doubles(maxa):
    return 2 * (maxa * (maxa + 1) // 2) + 6 * maxa + maxa * QP_MAXCG + 2 + (5 * maxa + 1) // 2 + 2


def test_table_covers_the_layouts(rows):
    for want in (lambda r: r["ngrp"] == 1, lambda r: r["ngrp"] > 1, lambda r: r["tw"], lambda r: not r["tw"], lambda r: r["nfo"], lambda r: not r["nfo"],
                 lambda r: r["nC"] % 2, lambda r: r["ncnln"] % 2, lambda r: r["P"] % 64, lambda r: r["qa"] == 32, lambda r: r["ja"] != r["jb"]):
        assert any(want(r) for r in rows)
    assert {r["nt"] for r in rows} == {128, 256, 512} and {r["qp"] for r in rows} == {0, 1}


def test_workspace_is_nwt_doubles(rows):
    """plan_solve.cpp, nwt_doubles (per problem)"""
    for r in rows:
        rev = r["ngrp"] * (16 * r["jb"] + 48) * (r["hb"] + 1) if r["tw"] else 0
        qa = qp_maxa(r["ngrp"], r["nt"])
        qp = qa * ((r["nC"] + 1) & ~1) + ((r["ncnln"] + 1) & ~1) * (3 + r["cg"] + qa) if r["qp"] else 0
        assert r["total"] == r["ngrp"] * r["ng"] * (r["hb"] + 1) + rev + r["ngrp"] * r["P"] * r["cg"] * r["cg"] + qp, r


def test_lds_is_the_layouts(rows):
    """layout.cpp, ntg_make_layout: the area behind SmemLayout::nwt_y and the reduction scratch"""
    for r in rows:
        vec = 16 * (r["ja"] + 3) + 48 + 16 * (r["jb"] + 3) + 48 if r["tw"] else 16 * ((r["ng"] + 15) // 16) + 48
        steady = r["ngrp"] * (vec + (2 if r["tw"] else 1) * NWT_PANEL) * 8 + r["nfo"] * (16 * ((r["ngf"] + 15) // 16) + 48) * 8
        if r["qp"]:
            steady += (r["ngrp"] * qp_doubles(qp_maxa(r["ngrp"], r["nt"])) + QP_RED) * 8
        refresh = (r["nt"] // 64) * NWT_STAGE * 8 + r["ngrp"] * ((r["P"] + 63) // 64) * 8
        assert r["bytes"] == max(steady, refresh), r
        assert r["red_doubles"] * 8 == (32 * (r["nt"] // 64) + 2) * 8


def test_offsets_are_the_kernels(rows):
    """sqp_kernel's own statement: nwt_ksz, qp_pp, nwt_lena / lenb, nwt_yall, nwt_npan, the free outputs' vectors, qpbase, qpred, qp_c .. qp_JU,
    the block-flag words behind the staging buffers, nwt_flag"""
    for r in rows:
        npad, ncq, qa = (r["nC"] + 1) & ~1, (r["ncnln"] + 1) & ~1, qp_maxa(r["ngrp"], r["nt"])
        ksz = r["ngrp"] * r["ng"] * (r["hb"] + 1) + (r["ngrp"] * (16 * r["jb"] + 48) * (r["hb"] + 1) if r["tw"] else 0)
        assert (r["npad"], r["ncq"], r["qa"], r["qpd"]) == (npad, ncq, qa, qp_doubles(qa))
        assert r["Kb"] == r["ngrp"] * r["ng"] * (r["hb"] + 1) and r["B"] == ksz and r["U"] == ksz + r["ngrp"] * r["P"] * r["cg"] ** 2
        if r["qp"]:
            assert r["lamq"] == r["U"] + qa * npad and r["c"] == r["lamq"] + ncq and r["jwg"] == r["c"] + ncq and r["a"] == r["jwg"] + ncq
            assert r["JU"] == r["a"] + ncq * r["cg"] and r["total"] == r["JU"] + ncq * qa
        else:
            assert r["U"] == r["lamq"] == r["c"] == r["jwg"] == r["a"] == r["JU"] == r["total"]
        lena, lenb, ylen = 16 * (r["ja"] + 3) + 48, 16 * (r["jb"] + 3) + 48, 16 * ((r["ng"] + 15) >> 4) + 48
        yall = r["ngrp"] * (lena + lenb if r["tw"] else ylen)
        assert (r["lena"], r["lenb"], r["ylen"], r["yb"], r["panel"], r["npan"]) == (lena, lenb, ylen, r["ngrp"] * lena, yall, (2 if r["tw"] else 1) * r["ngrp"])
        ylenf = 16 * ((r["ngf"] + 15) >> 4) + 48
        assert (r["yf"], r["ylenf"]) == (yall + r["npan"] * NWT_PANEL, ylenf)
        assert r["slots"] == yall + r["npan"] * NWT_PANEL + r["nfo"] * ylenf and r["red"] == r["slots"] + r["ngrp"] * r["qpd"]
        assert r["act"] == (r["nt"] // 64) * NWT_STAGE and r["flag"] == 2 * (32 * (r["nt"] // 64) + 2) - 2


def test_areas_follow_one_another_and_end_at_the_totals(rows):
    for r in rows:
        # workspace: bands, reversed arrays, blocks, then the QP's arrays
        sizes = [r["Kb"], r["B"] - r["Kb"], r["ngrp"] * r["P"] * r["cg"] ** 2]
        starts = [0, r["Kb"], r["B"]]
        if r["qp"]:
            starts += [r["U"], r["lamq"], r["c"], r["jwg"], r["a"], r["JU"]]
            sizes += [r["qa"] * r["npad"], r["ncq"], r["ncq"], r["ncq"], r["ncq"] * r["cg"], r["ncq"] * r["qa"]]
        for s, n, nxt in zip(starts, sizes, starts[1:] + [r["total"]]):
            assert s + n == nxt, r
        # LDS between refreshes: solve vectors (a parts, b parts), panels, free outputs' vectors, slots, search scratch
        vec = [(0, r["ngrp"] * r["lena"]), (r["yb"], r["ngrp"] * r["lenb"])] if r["tw"] else [(0, r["ngrp"] * r["ylen"])]
        areas = vec + [(r["panel"], r["npan"] * NWT_PANEL), (r["yf"], r["nfo"] * r["ylenf"])]
        if r["qp"]:
            areas += [(r["slots"], r["ngrp"] * r["qpd"]), (r["red"], QP_RED)]
        end = 0
        for s, n in areas:
            assert s == end, r
            end = s + n
        # ... and inside a refresh: staging buffers, block-flag words
        end2 = r["act"] + r["ngrp"] * ((r["P"] + 63) // 64)
        assert r["act"] == (r["nt"] // 64) * NWT_STAGE and max(end, end2) * 8 == r["bytes"], r
        # the flag word pair is the last double of the reduction scratch, behind block_sum's two halves of 16 values per wave
        assert r["flag"] % 2 == 0 and r["flag"] // 2 == r["red_doubles"] - 1 >= 32 * (r["nt"] // 64)

"""tools/pmc_by_layer.py on synthetic inputs (CPU): the library's launch log and rocprofv3's per-dispatch counter rows are joined by dispatch order,
dispatches the library does not log are skipped (and counted), launches that share a label but differ in size are averaged, and the per-engine
groups that bench.py's training leg reads come out of the same join."""
import csv
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_pass(d, counter, values):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "1_counter_collection.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value", "Start_Timestamp", "End_Timestamp"])
        for i, (kernel, v, dur) in enumerate(values, 1):
            for xcd_share in (0.5, 0.5):  # rocprofv3 writes one row per XCD group: the tool sums them per dispatch
                w.writerow([i, kernel, counter, v * xcd_share, 1000 * i, 1000 * i + dur])
            w.writerow([i, kernel, "SOMETHING_ELSE", 7, 1000 * i, 1000 * i + dur])


def test_join_by_dispatch_order_and_groups(tmp_path):
    disp = [("void hificar::front_kernel(hificar::FrontParams)", 10.0, 100),
            ("void hificar::conv_f32do_kernel<4, 1, 4, 4>(hificar::MultiConvParams)", 1000.0, 2000),
            ("void hificar::loss_reduce_kernel(hificar::LossEntry const*)", 1.0, 10),           # not in the log: skipped, counted
            ("void hificar::conv_f32do_kernel<4, 1, 4, 4>(hificar::MultiConvParams)", 3000.0, 4000),
            ("void hificar::im2col4_kernel(hificar::Im2colParams)", 50.0, 100),                   # logged under its scalar sibling's family name
            ("void hificar::pack_all_kernel(hificar::PackParams const*, int const*, int)", 100.0, 300),
            ("void hificar::pack_all_kernel(hificar::PackParams const*, int const*, int)", 300.0, 500),
            ("at::native::something_else()", 5.0, 5)]
    log = ["front_kernel\t0\t1000", "conv_f32do_kernel<4,1,4,4>|blocks.2.convs1.0.1 x3\t2e9\t1024000",
           "conv_f32do_kernel<4,1,4,4>|mpd.discriminators.1.convs.4.0#g0 x1\t4e9\t1024000", "im2col_kernel|mpd.discriminators.1.convs.4.0\t0\t51200",
           "pack_all_kernel\t0\t102400", "pack_all_kernel\t0\t307200"]
    for name, ctr in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE")):
        _write_pass(str(tmp_path / name), ctr, disp)
        (tmp_path / f"{name}.log").write_text("\n".join(log) + "\n")
    out, gj = tmp_path / "t.csv", tmp_path / "g.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pmc_by_layer.py"), "--fetch", str(tmp_path / "fetch"), "--fetch-log", str(tmp_path / "fetch.log"),
                        "--write", str(tmp_path / "write"), "--write-log", str(tmp_path / "write.log"), "--out", str(out), "--groups-json", str(gj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "6 launches joined, 1 unlogged dispatches {'loss_reduce_kernel': 1}, 0 log entries without a dispatch" in r.stderr
    rows = {(x["Kernel"], x["Layer"]): x for x in csv.DictReader(ln for ln in open(out) if not ln.startswith("#"))}
    gen = rows[("conv_f32do_kernel<4,1,4,4>", "blocks.2.convs1.0.1 x3")]
    # FETCH 1000 KiB raw, WRITE 1000 KiB -> (2 * 1000 + 1000) * 1024 bytes against 1 024 000 algorithmic
    assert float(gen["FETCH_KiB_raw"]) == 1000.0 and float(gen["HBM_MB_corrected"]) == 3.07 and float(gen["traffic_over_algorithmic"]) == 3.0
    assert float(gen["avg_duration_us"]) == 2.0 and float(gen["TFLOP_s"]) == 1000.0
    assert float(rows[("conv_f32do_kernel<4,1,4,4>", "mpd.discriminators.1.convs.4.0#g0 x1")]["traffic_over_algorithmic"]) == 9.0
    assert ("im2col4_kernel", "mpd.discriminators.1.convs.4.0") in rows
    pk = rows[("pack_all_kernel", "")]  # two launches of different size under one label: averaged per launch
    assert int(pk["Launches"]) == 2 and float(pk["algorithmic_MB"]) == 0.2 and float(pk["FETCH_KiB_raw"]) == 200.0
    g = json.load(open(gj))
    assert g["generator convs (forward x2, data gradients)"]["launches"] == 1
    assert g["period discriminators (convs, im2col / col2im)"]["launches"] == 2
    assert g["conv_f32do_kernel @ period discriminators (convs, im2col / col2im)"]["traffic_over_algorithmic"] == 9.0
    assert g["other (reductions, packs, losses, element-wise)"]["launches"] == 3  # front_kernel + the two packs


def test_weight_gradient_detail_labels_join_by_family(tmp_path):
    """With HIFICAR_PROFILE_DETAIL the weight-gradient label carries the instantiation ("wgrad_taps_kernel<7,0,128> shape sS rR nN") and the
    deferred reduction its counts ("reduce_multi_kernel wN bM"): both still join with rocprofv3's names by family, the rest of the label is the layer."""
    disp = [("void hificar::front_kernel(hificar::FrontParams)", 10.0, 100),
            ("void hificar::wgrad_taps_kernel<7, false, 128>(hificar::WgradTapsPair)", 200.0, 400),
            ("void hificar::wgrad_gemm_kernel<4, 32>(hificar::WgradTapsPair)", 400.0, 800),
            ("void hificar::wgrad_kernel(hificar::WgradParams)", 100.0, 200),
            ("void hificar::reduce_multi_kernel(hificar::ReduceTable)", 20.0, 50)]
    log = ["front_kernel\t0\t1000", "wgrad_taps_kernel<7,0,128> 48x48k5p1 s3 r1 n2\t1e9\t204800", "wgrad_gemm_kernel<4,32> 256x256k1p1 s6 r1 n1\t2e9\t409600",
           "wgrad_kernel 48x48k13p1 s6 r1 n1\t1e9\t102400", "reduce_multi_kernel w3 b3\t0\t20480"]
    for name, ctr in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE")):
        _write_pass(str(tmp_path / name), ctr, disp)
        (tmp_path / f"{name}.log").write_text("\n".join(log) + "\n")
    out, gj = tmp_path / "t.csv", tmp_path / "g.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pmc_by_layer.py"), "--fetch", str(tmp_path / "fetch"), "--fetch-log", str(tmp_path / "fetch.log"),
                        "--write", str(tmp_path / "write"), "--write-log", str(tmp_path / "write.log"), "--out", str(out), "--groups-json", str(gj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "5 launches joined, 0 unlogged dispatches {}, 0 log entries without a dispatch" in r.stderr
    rows = {(x["Kernel"], x["Layer"]): x for x in csv.DictReader(ln for ln in open(out) if not ln.startswith("#"))}
    assert ("wgrad_taps_kernel<7,false,128>", "48x48k5p1 s3 r1 n2") in rows and ("wgrad_gemm_kernel<4,32>", "256x256k1p1 s6 r1 n1") in rows
    assert ("wgrad_kernel", "48x48k13p1 s6 r1 n1") in rows and ("reduce_multi_kernel", "w3 b3") in rows
    g = json.load(open(gj))
    assert g["weight gradients"]["launches"] == 3 and g["wgrad_taps_kernel @ weight gradients"]["launches"] == 1
    assert g["other (reductions, packs, losses, element-wise)"]["launches"] == 2  # front_kernel and the reduction


def test_gather_width_suffix_joins_by_family(tmp_path):
    """With HIFICAR_PROFILE_DETAIL the discriminators' gather labels say which kernel ran ("im2col_kernel|layer v4", "col2im_mask_kernel|layer v1"):
    they still join with rocprofv3's names by family (the 4-wide kernels under their scalar siblings'), and the layer keeps its engine."""
    disp = [("void hificar::front_kernel(hificar::FrontParams)", 10.0, 100),
            ("void hificar::im2col4_kernel(hificar::Im2colParams)", 50.0, 100),
            ("void hificar::im2col_kernel(hificar::Im2colParams)", 60.0, 120),
            ("void hificar::col2im_mask4_kernel(hificar::Col2imParams)", 70.0, 140),
            ("void hificar::col2im_mask_kernel(hificar::Col2imParams)", 80.0, 160)]
    log = ["front_kernel\t0\t1000", "im2col_kernel|msd.discriminators.0.layers.1.0 v4\t0\t51200", "im2col_kernel|mpd.discriminators.1.convs.1.0 v1\t0\t51200",
           "col2im_mask_kernel|msd.discriminators.0.layers.0.0 v4\t0\t51200", "col2im_mask_kernel|mpd.discriminators.1.convs.0.0 v1\t0\t51200"]
    for name, ctr in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE")):
        _write_pass(str(tmp_path / name), ctr, disp)
        (tmp_path / f"{name}.log").write_text("\n".join(log) + "\n")
    out, gj = tmp_path / "t.csv", tmp_path / "g.json"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pmc_by_layer.py"), "--fetch", str(tmp_path / "fetch"), "--fetch-log", str(tmp_path / "fetch.log"),
                        "--write", str(tmp_path / "write"), "--write-log", str(tmp_path / "write.log"), "--out", str(out), "--groups-json", str(gj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "5 launches joined, 0 unlogged dispatches {}, 0 log entries without a dispatch" in r.stderr
    rows = {(x["Kernel"], x["Layer"]): x for x in csv.DictReader(ln for ln in open(out) if not ln.startswith("#"))}
    assert ("im2col4_kernel", "msd.discriminators.0.layers.1.0 v4") in rows and ("im2col_kernel", "mpd.discriminators.1.convs.1.0 v1") in rows
    assert ("col2im_mask4_kernel", "msd.discriminators.0.layers.0.0 v4") in rows and ("col2im_mask_kernel", "mpd.discriminators.1.convs.0.0 v1") in rows
    g = json.load(open(gj))
    assert g["scale discriminators (convs, im2col / col2im)"]["launches"] == 2 and g["period discriminators (convs, im2col / col2im)"]["launches"] == 2
    assert g["im2col_kernel @ scale discriminators (convs, im2col / col2im)"]["launches"] == 1
    assert g["col2im_mask_kernel @ period discriminators (convs, im2col / col2im)"]["launches"] == 1

"use strict";
// Text reads through the Node surface: documents of a log replayed into BatchClients that follow the
// executed steps of tests/golden/textreads.expected.jsonl (make_textreads.py) through
// createTextHelper() -- getText / getTextAndMarkers in the recorded views -- and, for the reads of the
// client's own view, through the SharedString readers of BatchClient; one JSON line per document
// {doc, err, steps: [[outputs per op]], strings: [[marker strings per "*" op]], plain}.
// A "*" read's text carries Marker.toString()s whose properties are in the host's key order (the
// reference's is their insertion order): `strings` are this host's, and the text is reported with each
// replaced by the recorded one when the two are equal up to that order.
//   node replay_textreads.js <log.mtlog> <fixture.jsonl> <log name> <n docs> [tileKey]
const fs = require("fs");
const { BatchEngine } = require("./batchClient.js");
const { markerToString } = require("./textHelper.js");
const { loadLog, messages } = require("./mtlog.js");

const log = loadLog(process.argv[2]);
const name = process.argv[4], nDocs = parseInt(process.argv[5], 10);
const opts = process.argv[6] !== undefined ? { tileKey: parseInt(process.argv[6], 10) } : undefined;
const rows = fs.readFileSync(process.argv[3], "utf8").split("\n").filter((x) => x).map((x) => JSON.parse(x))
    .filter((r) => r.log === name && r.doc < nDocs);
const eng = new BatchEngine({ maxDocs: rows.length, opsPerLaunch: 16 });
const sorted = (v) => (Array.isArray(v) ? v.map(sorted) : v && typeof v === "object"
    ? Object.keys(v).sort().reduce((o, k) => { o[k] = sorted(v[k]); return o; }, {}) : v);
const parts = (s) => { const at = s.indexOf("{"); return at < 0 ? [s, null] : [s.slice(0, at), JSON.stringify(sorted(JSON.parse(s.slice(at))))]; };
const out = [];
for (const row of rows) {
    const items = [...messages(log, row.doc, opts)];
    const own = items.find((x) => x.local);
    const c = eng.createClient();
    c.startOrUpdateCollaboration(own ? "c" + own.client : "observer");
    const helper = c.createTextHelper();
    const steps = [];
    let err = null, si = 0, plain = true;
    const step = (st) => {
        const outs = [];
        for (const op of st.ops) {
            const view = op[1], s = op[3] === null ? undefined : op[3], e = op[4] === null ? undefined : op[4];
            const refSeq = view ? view[0] : c.getCurrentSeq(), clientId = view ? c._shortId("c" + view[1]) : c.getClientId();
            if (op[0] === "m") {
                const r = helper.getTextAndMarkers(refSeq, clientId, op[2], s, e);
                if (!view && s === undefined && e === undefined) {
                    const mine = c.getTextAndMarkers(op[2]);
                    if (JSON.stringify(mine.parallelText) !== JSON.stringify(r.parallelText)) throw new Error("BatchClient.getTextAndMarkers");
                }
                outs.push([r.parallelText, r.parallelMarkers.map((m) => m.ordinal)]);
                continue;
            }
            let text = helper.getText(refSeq, clientId, op[2], s, e);
            if (!view) {  // the SharedString readers answer the same reads of the client's own view
                const mine = op[2] === "" ? (s === undefined ? c.getText() : c.getText(s, e))
                    : op[2] === " " ? (s === undefined ? c.getTextWithPlaceholders() : c.getTextRangeWithPlaceholders(s, e))
                        : (s === undefined ? text : c.getTextRangeWithMarkers(s, e));
                if (mine !== text) throw new Error(`BatchClient reader (${JSON.stringify(op.slice(0, 5))}): ${JSON.stringify(mine)} != ${JSON.stringify(text)}`);
            }
            if (op[2] === "*") {
                // the recorded marker strings (the last field of the op) against this host's, in order
                const want = op[op.length - 1];
                let at = 0, rebuilt = "";
                for (const w of want) {
                    const nl = text.indexOf("\n" + parts(w)[0], at);
                    if (nl < 0) throw new Error(`"*": marker ${JSON.stringify(w)} not found in ${JSON.stringify(text)}`);
                    // this host's string runs to where its properties' JSON ends
                    const [head, props] = parts(w);
                    let end = nl + 1 + head.length;
                    if (props !== null) {
                        let depth = 0, k = end, str = false;
                        for (; k < text.length; k++) {
                            const ch = text[k];
                            if (str) { if (ch === "\\") k++; else if (ch === "\"") str = false; continue; }
                            if (ch === "\"") str = true;
                            else if (ch === "{" || ch === "[") depth++;
                            else if ((ch === "}" || ch === "]") && --depth === 0) { k++; break; }
                        }
                        if (JSON.stringify(sorted(JSON.parse(text.slice(end, k)))) !== props) throw new Error(`"*": properties of ${JSON.stringify(w)}`);
                        end = k;
                    }
                    rebuilt += text.slice(at, nl) + "\n" + w;
                    at = end;
                }
                text = rebuilt + text.slice(at);
            }
            outs.push([text]);
        }
        steps.push(outs);
    };
    try {
        while (si < row.steps.length && row.steps[si].k === 0) step(row.steps[si++]);
        for (const it of items) {
            if (it.regen) {
                c.regeneratePendingOp(it.op);
            } else if (it.local) {
                const op = it.op;
                if (op.type === 0) {
                    if (typeof op.seg === "string") c.insertTextLocal(op.pos1, op.seg);
                    else if (op.seg.marker) c.insertMarkerLocal(op.pos1, op.seg.marker.refType, op.seg.props);
                    else c.insertTextLocal(op.pos1, op.seg.text, op.seg.props);
                } else if (op.type === 1) {
                    c.removeRangeLocal(op.pos1, op.pos2);
                } else {
                    c.annotateRangeLocal(op.pos1, op.pos2, op.props, op.combiningOp);
                }
            } else {
                c.applyMsg(it);
            }
            while (si < row.steps.length && row.steps[si].k === it.end) step(row.steps[si++]);
        }
        // getText() without arguments: the whole-document read, the same as the ranged read of everything
        plain = c.getText() === helper.getText(c.getCurrentSeq(), c.getClientId(), "", 0, 2147483647) && typeof markerToString === "function";
    } catch (e) {
        err = String(e.stack || e.message || e);
    }
    out.push(JSON.stringify({ doc: row.doc, err, steps, plain }));
}
process.stdout.write(out.join("\n") + "\n");

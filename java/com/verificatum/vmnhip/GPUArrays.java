package com.verificatum.vmnhip;

import java.nio.ByteBuffer;

import com.verificatum.arithm.PGroupElementArray;
import com.verificatum.arithm.PPGroupElementArray;
import com.verificatum.arithm.PRingElementArray;
import com.verificatum.arithm.Permutation;
import com.verificatum.eio.ByteTreeBasic;

/** Conversions between VCR's host objects and the device arrays: uploads go through the array's byte tree (the format
 *  the library parses on the GPU, SURVEY.md App. D), ciphertext arrays are split into their 2 * width component arrays
 *  (struct of arrays, the way {@code PPGroupElementArray.project} exposes them,
 *  src/java/com/verificatum/protocol/elgamal/DistrElGamalSession.java:377-378), permutations become gather tables. */
final class GPUArrays {
    private GPUArrays() { }

    /** The gather table of X.permute(pi): VCR puts X[i] at position pi.map(i), so out[k] = X[pi^-1(k)]. */
    static int[] gatherTable(final Permutation pi) {
        final Permutation inv = pi.inv();
        final int[] table = new int[inv.size()];
        for (int i = 0; i < table.length; i++) {
            table[i] = inv.map(i);
        }
        return table;
    }

    /** {@code Permutation.random(n, randomSource, rbitlen)} drawn on the device from one PRG seed (32 / 48 / 64 bytes of the
     *  party's RandomSource; vmn_permutation_from_prg, the rule is stated in csrc/permutation_layout.h): the result is used
     *  where {@link #gatherTable} of a host permutation would be -- out[k] = X[table[k]].  The inverse of a uniform
     *  permutation is uniform, so the table is the secret permutation itself; no host Permutation object is built. */
    static int[] randomPermutation(final GPUGroup group, final byte[] seed, final int n, final int rbitlen) {
        final int[] table = new int[n];
        VMNException.check(VMNHip.vmn_permutation_from_prg(group.ctx, seed, seed.length, n, rbitlen, table, null));
        return table;
    }

    static ByteBuffer direct(final ByteTreeBasic bt) {
        final byte[] bytes = bt.toByteArray();
        final ByteBuffer buf = ByteBuffer.allocateDirect(bytes.length);
        buf.put(bytes);
        buf.flip();
        return buf;
    }

    /** The payload bytes of an element's byte tree: leaf -> its bytes; node(leaf, leaf) (a curve point) -> x || y. */
    static byte[] leafPayload(final ByteTreeBasic bt, final int elemBytes) {
        final byte[] raw = bt.toByteArray();
        final byte[] out = new byte[elemBytes];
        if (raw[0] == 1) {
            System.arraycopy(raw, 5, out, 0, elemBytes);
        } else {
            final int half = elemBytes / 2;
            System.arraycopy(raw, 5 + 5, out, 0, half);
            System.arraycopy(raw, 5 + 5 + half + 5, out, half, half);
        }
        return out;
    }

    static PGroupElementArrayGPU upload(final GPUGroup group, final PGroupElementArray a) {
        final ByteBuffer buf = direct(a.toByteTree());
        return PGroupElementArrayGPU.fromByteTree(group, buf, buf.remaining(), a.size());
    }

    static PRingElementArrayGPU upload(final GPUGroup group, final PRingElementArray a) {
        final ByteBuffer buf = direct(a.toByteTree());
        final long[] out = new long[1];
        final int[] formatOk = new int[1];
        final int[] inRange = new int[1];
        VMNException.check(VMNHip.vmn_rarray_from_bytetreeDirect(group.grp, buf, buf.remaining(), a.size(), out, formatOk, inRange));
        if (formatOk[0] == 0 || inRange[0] == 0) {
            throw new VMNException(VMNException.ERR_FORMAT);
        }
        return new PRingElementArrayGPU(group, out[0]);
    }

    /** A ciphertext array of width w as its 2w component arrays [u_1..u_w, v_1..v_w]. */
    static PGroupElementArrayGPU[] components(final GPUGroup group, final PGroupElementArray ciphertexts, final int width) {
        final PPGroupElementArray pp = (PPGroupElementArray) ciphertexts;
        final PGroupElementArrayGPU[] out = new PGroupElementArrayGPU[2 * width];
        for (int half = 0; half < 2; half++) {
            final PGroupElementArray part = pp.project(half);
            for (int c = 0; c < width; c++) {
                final PGroupElementArray col = width == 1 ? part : ((PPGroupElementArray) part).project(c);
                out[half * width + c] = upload(group, col);
            }
        }
        return out;
    }

    /** A list in the reference's {@code native} interface (one ciphertext per line, the line the hexadecimal byte tree of that
     *  ciphertext: CiphertextReaderLine) as its 2w component arrays [u_1..u_w, v_1..v_w], parsed on the GPU.  {@code text}: a
     *  direct buffer holding the file, {@code len} its bytes; {@code expectedSize} 0 accepts any number of lines.  A malformed
     *  line, a value out of range or an element outside the group is the reference's ArithmFormatException / EIOException;
     *  {@code firstBadLine} (may be null) receives the zero-based index of the first malformed line. */
    static PGroupElementArrayGPU[] readCiphertextsNative(final GPUGroup group, final ByteBuffer text, final long len, final int width,
                                                         final long expectedSize, final long[] firstBadLine) {
        final long[] out = new long[2 * width];
        final long[] lines = new long[1];
        final long[] bad = new long[1];
        final int[] formatOk = new int[1];
        final int[] inRange = new int[1];
        VMNException.check(VMNHip.vmn_garrays_from_hexlinesDirect(group.grp, width, text, len, expectedSize, out, lines, formatOk, bad, inRange));
        return listOrException(group, out, formatOk[0], bad[0], inRange[0], firstBadLine);
    }

    /** readCiphertextsNative under a public key of width {@code keyWidth} (ProtocolElGamal.java:476-481): the plaintext group is
     *  G^keyWidth, every half of a line is nested once more, and the list comes as its 2 * keyWidth * width component arrays in
     *  flat order, the u half first, component l * keyWidth + j the key j of plaintext component l.  keyWidth 1 is
     *  readCiphertextsNative. */
    static PGroupElementArrayGPU[] readCiphertextsNativeKeyed(final GPUGroup group, final ByteBuffer text, final long len,
                                                              final int keyWidth, final int width, final long expectedSize,
                                                              final long[] firstBadLine) {
        final long[] out = new long[2 * keyWidth * width];
        final long[] lines = new long[1];
        final long[] bad = new long[1];
        final int[] formatOk = new int[1];
        final int[] inRange = new int[1];
        VMNException.check(VMNHip.vmn_garrays_from_hexlines_keyedDirect(group.grp, keyWidth, width, text, len, expectedSize, out, lines,
                                                                        formatOk, bad, inRange));
        return listOrException(group, out, formatOk[0], bad[0], inRange[0], firstBadLine);
    }

    /** The policy of both line interfaces on what a reader returned: a format defect, a value out of range or an element
     *  outside the group is no list. */
    private static PGroupElementArrayGPU[] listOrException(final GPUGroup group, final long[] out, final int formatOk, final long bad,
                                                           final int inRange, final long[] firstBadLine) {
        if (firstBadLine != null) {
            firstBadLine[0] = bad;
        }
        if (formatOk == 0) {
            throw new VMNException(VMNException.ERR_FORMAT);
        }
        final PGroupElementArrayGPU[] comps = new PGroupElementArrayGPU[out.length];
        for (int c = 0; c < comps.length; c++) {
            comps[c] = new PGroupElementArrayGPU(group, out[c]);
        }
        boolean ok = inRange != 0;
        for (int c = 0; ok && c < comps.length; c++) {
            ok = comps[c].isMember();
        }
        if (!ok) {
            free(comps);
            throw new VMNException(VMNException.ERR_FORMAT);
        }
        return comps;
    }

    /** A list in the reference's {@code json} interface (ProtocolElGamalInterfaceJSONDecode: one ciphertext per line,
     *  {"alpha":"A","beta":"B"} with decimal strings, an array of such pairs at width > 1; modular groups only) as its 2w
     *  component arrays, parsed and converted from decimal on the GPU.  Arguments and exceptions as readCiphertextsNative. */
    static PGroupElementArrayGPU[] readCiphertextsJSON(final GPUGroup group, final ByteBuffer text, final long len, final int width,
                                                       final long expectedSize, final long[] firstBadLine) {
        final long[] out = new long[2 * width];
        final long[] lines = new long[1];
        final long[] bad = new long[1];
        final int[] formatOk = new int[1];
        final int[] inRange = new int[1];
        VMNException.check(VMNHip.vmn_garrays_from_jsonlinesDirect(group.grp, width, text, len, expectedSize, out, lines, formatOk, bad, inRange));
        return listOrException(group, out, formatOk[0], bad[0], inRange[0], firstBadLine);
    }

    /** The reverse (writeCiphertexts of the json interface): decimals without leading zeros, no spaces, every line ended by a
     *  newline, into a fresh direct buffer limited to the bytes written. */
    static ByteBuffer writeCiphertextsJSON(final GPUGroup group, final PGroupElementArrayGPU[] comps) {
        return jsonLines(group, comps, comps.length / 2, false);
    }

    /** decodePlaintexts of the json interface: line i is "M" (width 1) or ["M1",...,"Mw"], the decimal value of plaintext i. */
    static ByteBuffer decodePlaintextsJSON(final GPUGroup group, final PGroupElementArrayGPU[] plaintexts) {
        return jsonLines(group, plaintexts, plaintexts.length, true);
    }

    private static ByteBuffer jsonLines(final GPUGroup group, final PGroupElementArrayGPU[] arrays, final int width, final boolean plain) {
        final long[] h = handles(arrays);
        final long lines = arrays.length == 0 ? 0 : VMNHip.vmn_garray_size(h[0]);
        final long cap = Math.max(1L, lines * VMNHip.vmn_jsonlines_max_line_bytes(group.grp, width));
        final ByteBuffer buf = ByteBuffer.allocateDirect((int) cap);
        final long[] written = new long[1];
        VMNException.check(plain ? VMNHip.vmn_garrays_to_jsonplainDirect(h, width, buf, cap, written)
                                 : VMNHip.vmn_garrays_to_jsonlinesDirect(h, width, buf, cap, written));
        buf.limit((int) written[0]);
        return buf;
    }

    /** Lines of text as a list of plaintexts (pGroup.encode over a safe-prime group, include/vmnhip.h: vmn_garrays_from_textlines):
     *  line i, cut into pieces of vmn_group_encode_length bytes, is element i of the {@code ncomp} component arrays.  A line of more
     *  than ncomp times that many bytes is no list: {@code firstLongLine[0]} (may be null) receives its zero-based index and the
     *  call throws. */
    static PGroupElementArrayGPU[] encodePlaintexts(final GPUGroup group, final ByteBuffer text, final long len, final int ncomp,
                                                    final long[] firstLongLine) {
        final long[] out = new long[ncomp];
        final long[] lines = new long[1];
        final long[] longLine = new long[1];
        final int[] fits = new int[1];
        VMNException.check(VMNHip.vmn_garrays_from_textlinesDirect(group.grp, ncomp, text, len, out, lines, fits, longLine));
        if (firstLongLine != null) {
            firstLongLine[0] = longLine[0];
        }
        if (fits[0] == 0) {
            throw new VMNException(VMNException.ERR_FORMAT);
        }
        final PGroupElementArrayGPU[] comps = new PGroupElementArrayGPU[ncomp];
        for (int c = 0; c < ncomp; c++) {
            comps[c] = new PGroupElementArrayGPU(group, out[c]);
        }
        return comps;
    }

    /** decodePlaintexts of the native interface (ProtocolElGamalInterfaceString.java:197-236): line i is the message of plaintext
     *  i -- its components' messages one after the other -- without its \n and \r bytes, into a fresh direct buffer limited to
     *  the bytes written.  {@code verdicts} (may be null) receives {all well-formed, all UTF-8}: an element that holds no
     *  message gives an empty piece, a line that is not UTF-8 is written byte for byte. */
    static ByteBuffer decodePlaintextsNative(final GPUGroup group, final PGroupElementArrayGPU[] plaintexts, final boolean[] verdicts) {
        final long[] h = handles(plaintexts);
        final long lines = plaintexts.length == 0 ? 0 : VMNHip.vmn_garray_size(h[0]);
        final long cap = Math.max(1L, lines * (plaintexts.length * VMNHip.vmn_group_encode_length(group.grp) + 1));
        final ByteBuffer buf = ByteBuffer.allocateDirect((int) cap);
        final long[] written = new long[1];
        final int[] wellformed = new int[1];
        final int[] utf8 = new int[1];
        VMNException.check(VMNHip.vmn_garrays_to_textlinesDirect(h, plaintexts.length, buf, cap, written, wellformed, utf8));
        if (verdicts != null) {
            verdicts[0] = wellformed[0] != 0;
            verdicts[1] = utf8[0] != 0;
        }
        buf.limit((int) written[0]);
        return buf;
    }

    /** The reverse (CiphertextWriterLine): lowercase digits, every line ended by a newline, into a fresh direct buffer. */
    static ByteBuffer writeCiphertextsNative(final PGroupElementArrayGPU[] comps) {
        final long[] h = handles(comps);
        final int width = comps.length / 2;
        final long size = VMNHip.vmn_garrays_hexlines_size(h, width);
        final ByteBuffer buf = ByteBuffer.allocateDirect((int) Math.max(1L, size));
        VMNException.check(VMNHip.vmn_garrays_to_hexlinesDirect(h, width, buf));
        buf.limit((int) size);
        return buf;
    }

    /** writeCiphertextsNative for the 2 * keyWidth * width component arrays of a list under a public key of width
     *  {@code keyWidth}, in the order readCiphertextsNativeKeyed returns them. */
    static ByteBuffer writeCiphertextsNativeKeyed(final PGroupElementArrayGPU[] comps, final int keyWidth) {
        final long[] h = handles(comps);
        final int width = comps.length / (2 * keyWidth);
        final long size = VMNHip.vmn_garrays_hexlines_size_keyed(h, keyWidth, width);
        final ByteBuffer buf = ByteBuffer.allocateDirect((int) Math.max(1L, size));
        VMNException.check(VMNHip.vmn_garrays_to_hexlines_keyedDirect(h, keyWidth, width, buf));
        buf.limit((int) size);
        return buf;
    }

    static long[] handles(final PGroupElementArrayGPU[] arrays) {
        final long[] h = new long[arrays.length];
        for (int i = 0; i < h.length; i++) {
            h[i] = arrays[i].handle;
        }
        return h;
    }

    static long[] handles(final PRingElementArrayGPU[] arrays) {
        final long[] h = new long[arrays.length];
        for (int i = 0; i < h.length; i++) {
            h[i] = arrays[i].handle;
        }
        return h;
    }

    static void free(final PGroupElementArrayGPU[] arrays) {
        for (final PGroupElementArrayGPU a : arrays) {
            a.free();
        }
    }
}

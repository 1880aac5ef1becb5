! Capture wrapper for tests/golden/make_golden_therm_itd.py: bind(C) routines that set the module variables the public
! procedures of the reference's ice_therm_itd (and shift_ice of ice_itd) read, and call them on arrays handed in.
! Compiled against the module files of the reference build (oracle/build_ref.sh, configuration small) into a temporary
! library; nothing of it is committed but this text.
      module therm_itd_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine cap_set (ntr, dep, i_tsfc, i_iage, i_alvl, i_vlvl, l_iage, l_lvl, l_upd, hmax, himin, diag, ldiag) &
                 bind(C, name='cap_set')
      use ice_state, only: ntrcr, trcr_depend, nt_Tsfc, nt_iage, nt_alvl, nt_vlvl
      use ice_age, only: tr_iage
      use ice_mechred, only: tr_lvl
      use ice_flux, only: update_ocn_f
      use ice_itd, only: hin_max, hi_min, ilyr1, slyr1
      use ice_fileunits, only: nu_diag
      integer(c_int), value :: ntr, i_tsfc, i_iage, i_alvl, i_vlvl, l_iage, l_lvl, l_upd, ldiag
      character(kind=c_char) :: diag(ldiag)   ! file that receives what the reference writes to nu_diag
      integer(c_int) :: dep(max_ntrcr)
      real(c_double) :: hmax(0:ncat)
      real(c_double), value :: himin
      integer :: n
      character(len=1024) :: fname
      logical, save :: opened = .false.
      ntrcr = ntr
      trcr_depend(:) = dep(:)
      nt_Tsfc = i_tsfc; nt_iage = i_iage; nt_alvl = i_alvl; nt_vlvl = i_vlvl
      tr_iage = l_iage /= 0; tr_lvl = l_lvl /= 0; update_ocn_f = l_upd /= 0
      hin_max(:) = hmax(:)
      if (himin /= hi_min) stop 'cap_set: hi_min is a parameter of ice_itd (0.01)'
      do n = 1, ncat
         ilyr1(n) = (n-1)*nilyr + 1
         slyr1(n) = (n-1)*nslyr + 1
      enddo
      if (.not. opened) then
         nu_diag = 97
         fname = ' '
         do n = 1, min(ldiag, 1024)
            fname(n:n) = diag(n)
         enddo
         open (nu_diag, file=trim(fname), form='formatted')
         opened = .true.
      endif
      end subroutine cap_set

      subroutine cap_flush
      use ice_fileunits, only: nu_diag
      flush (nu_diag)
      end subroutine cap_flush

      subroutine cap_linear_itd (icells, indxi, indxj, aicen_init, vicen_init, aicen, trcrn, vicen, vsnon, &
                 eicen, esnon, aice, aice0, lstop, istop, jstop) bind(C, name='cap_linear_itd')
      use ice_state, only: ntrcr, trcr_depend
      use ice_therm_itd, only: linear_itd
      integer(c_int), value :: icells
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block), lstop, istop, jstop
      real(c_double) :: aicen_init(nx_block,ny_block,ncat), vicen_init(nx_block,ny_block,ncat), &
         aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), vicen(nx_block,ny_block,ncat), &
         vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), esnon(nx_block,ny_block,ntslyr), &
         aice(nx_block,ny_block), aice0(nx_block,ny_block)
      logical (kind=log_kind) :: l_stop
      call linear_itd (nx_block, ny_block, icells, indxi, indxj, ntrcr, trcr_depend(1:ntrcr), aicen_init, vicen_init, &
                       aicen, trcrn(:,:,1:ntrcr,:), vicen, vsnon, eicen, esnon, aice, aice0, l_stop, istop, jstop)
      lstop = merge(1, 0, l_stop)
      call cap_flush
      end subroutine cap_linear_itd

      subroutine cap_add_new_ice (icells, indxi, indxj, tmask, dt, aicen, trcrn, vicen, eicen, aice0, aice, frzmlt, &
                 frazil, frz_onset, yday, fresh, fsalt, Tf, lstop, istop, jstop) bind(C, name='cap_add_new_ice')
      use ice_state, only: ntrcr
      use ice_therm_itd, only: add_new_ice
      integer(c_int), value :: icells
      real(c_double), value :: dt, yday
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block), tmask(nx_block,ny_block), lstop, istop, jstop
      real(c_double) :: aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), &
         vicen(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), aice0(nx_block,ny_block), &
         aice(nx_block,ny_block), frzmlt(nx_block,ny_block), frazil(nx_block,ny_block), frz_onset(nx_block,ny_block), &
         fresh(nx_block,ny_block), fsalt(nx_block,ny_block), Tf(nx_block,ny_block)
      logical (kind=log_kind) :: l_stop, lmask(nx_block,ny_block)
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      lmask = tmask /= 0
      allocate (tr(nx_block,ny_block,ntrcr,ncat))
      tr = trcrn(:,:,1:ntrcr,:)
      call add_new_ice (nx_block, ny_block, ntrcr, icells, indxi, indxj, lmask, dt, aicen, tr, vicen, eicen, aice0, &
                        aice, frzmlt, frazil, frz_onset, yday, fresh, fsalt, Tf, l_stop, istop, jstop)
      trcrn(:,:,1:ntrcr,:) = tr
      lstop = merge(1, 0, l_stop)
      end subroutine cap_add_new_ice

      subroutine cap_lateral_melt (ilo, ihi, jlo, jhi, dt, fresh, fsalt, fhocn, rside, meltl, aicen, vicen, vsnon, &
                 eicen, esnon) bind(C, name='cap_lateral_melt')
      use ice_therm_itd, only: lateral_melt
      integer(c_int), value :: ilo, ihi, jlo, jhi
      real(c_double), value :: dt
      real(c_double) :: fresh(nx_block,ny_block), fsalt(nx_block,ny_block), fhocn(nx_block,ny_block), &
         rside(nx_block,ny_block), meltl(nx_block,ny_block), aicen(nx_block,ny_block,ncat), &
         vicen(nx_block,ny_block,ncat), vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), &
         esnon(nx_block,ny_block,ntslyr)
      call lateral_melt (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, fresh, fsalt, fhocn, rside, meltl, aicen, vicen, &
                         vsnon, eicen, esnon)
      end subroutine cap_lateral_melt

      subroutine cap_shift_ice (icells, indxi, indxj, aicen, trcrn, vicen, vsnon, eicen, esnon, hicen, donor, daice, &
                 dvice, lstop, istop, jstop) bind(C, name='cap_shift_ice')
      use ice_state, only: ntrcr, trcr_depend
      use ice_itd, only: shift_ice
      integer(c_int), value :: icells
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block), donor(icells,ncat), lstop, istop, jstop
      real(c_double) :: aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), &
         vicen(nx_block,ny_block,ncat), vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), &
         esnon(nx_block,ny_block,ntslyr), hicen(icells,ncat), daice(icells,ncat), dvice(icells,ncat)
      logical (kind=log_kind) :: l_stop
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      allocate (tr(nx_block,ny_block,ntrcr,ncat))
      tr = trcrn(:,:,1:ntrcr,:)
      call shift_ice (nx_block, ny_block, indxi, indxj, icells, ntrcr, trcr_depend(1:ntrcr), aicen, tr, vicen, vsnon, &
                      eicen, esnon, hicen, donor, daice, dvice, l_stop, istop, jstop)
      trcrn(:,:,1:ntrcr,:) = tr
      lstop = merge(1, 0, l_stop)
      end subroutine cap_shift_ice

      end module therm_itd_capture
